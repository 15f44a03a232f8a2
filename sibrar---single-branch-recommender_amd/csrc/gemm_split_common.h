// Shared pieces of the bf16-split fp32 GEMM kernels (gemm_split_f32.hip, gemm_split_wide_f32.hip, gemm_split_tn_f32.hip): the exact
// three-way split of an fp32 number into bf16 numbers, the six-term multiply-accumulate, the operand loaders / plane stores, the
// accumulator layout and the launch helper. See the header of gemm_split_f32.hip for the arithmetic.
#pragma once
#include "gemm_args.h"

typedef __bf16 sp_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sp_bf16x2 __attribute__((ext_vector_type(2)));
typedef float sp_f32x2 __attribute__((ext_vector_type(2)));
typedef float sp_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned sp_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) sp_u32x4 sp_lds_u32x4;

__device__ __forceinline__ unsigned sp_pack(float x, float y) {     // two fp32 -> two bf16 (round to nearest even), x in the low half
  sp_f32x2 v = {x, y};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, sp_bf16x2));
}

// (x, y) -> three packed bf16 pairs with x = x0 + x1 + x2 exactly
__device__ __forceinline__ void sp_split2(float x, float y, unsigned& p0, unsigned& p1, unsigned& p2) {
  p0 = sp_pack(x, y);
  x -= __uint_as_float(p0 << 16);
  y -= __uint_as_float(p0 & 0xffff0000u);
  p1 = sp_pack(x, y);
  x -= __uint_as_float(p1 << 16);
  y -= __uint_as_float(p1 & 0xffff0000u);
  p2 = sp_pack(x, y);
}

__device__ __forceinline__ void sp_split8(const float4 lo, const float4 hi, sp_u32x4& p0, sp_u32x4& p1, sp_u32x4& p2) {
  unsigned a, b, c;
  sp_split2(lo.x, lo.y, a, b, c); p0[0] = a; p1[0] = b; p2[0] = c;
  sp_split2(lo.z, lo.w, a, b, c); p0[1] = a; p1[1] = b; p2[1] = c;
  sp_split2(hi.x, hi.y, a, b, c); p0[2] = a; p1[2] = b; p2[2] = c;
  sp_split2(hi.z, hi.w, a, b, c); p0[3] = a; p1[3] = b; p2[3] = c;
}

__device__ __forceinline__ sp_f32x16 sp_mfma(const sp_u32x4 a, const sp_u32x4 b, const sp_f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(sp_bf16x8, a), __builtin_bit_cast(sp_bf16x8, b), c, 0, 0, 0);
}

// acc += the six leading partial products of one A triple and one W triple (a[p], w[p]: plane p of the split), smallest terms first:
// (2,0) (0,2) (1,1) (1,0) (0,1) (0,0). The order is part of the results' bits.
__device__ __forceinline__ void sp_mac6(const sp_u32x4 (&a)[3], const sp_u32x4 (&w)[3], sp_f32x16& acc) {
  acc = sp_mfma(a[2], w[0], acc);
  acc = sp_mfma(a[0], w[2], acc);
  acc = sp_mfma(a[1], w[1], acc);
  acc = sp_mfma(a[1], w[0], acc);
  acc = sp_mfma(a[0], w[1], acc);
  acc = sp_mfma(a[0], w[0], acc);
}

// the same for two W triples and two accumulators, term by term: two independent chains, each MFMA behind one of the other chain
__device__ __forceinline__ void sp_mac6x2(const sp_u32x4 (&a)[3], const sp_u32x4 (&w0)[3], const sp_u32x4 (&w1)[3], sp_f32x16& acc0,
                                          sp_f32x16& acc1) {
  acc0 = sp_mfma(a[2], w0[0], acc0); acc1 = sp_mfma(a[2], w1[0], acc1);
  acc0 = sp_mfma(a[0], w0[2], acc0); acc1 = sp_mfma(a[0], w1[2], acc1);
  acc0 = sp_mfma(a[1], w0[1], acc0); acc1 = sp_mfma(a[1], w1[1], acc1);
  acc0 = sp_mfma(a[1], w0[0], acc0); acc1 = sp_mfma(a[1], w1[0], acc1);
  acc0 = sp_mfma(a[0], w0[1], acc0); acc1 = sp_mfma(a[0], w1[1], acc1);
  acc0 = sp_mfma(a[0], w0[0], acc0); acc1 = sp_mfma(a[0], w1[0], acc1);
}

__device__ __forceinline__ void sp_clear(sp_f32x16* acc, const int tiles) {
#pragma unroll
  for (int j = 0; j < tiles; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
}

// split 8 values and store their three bf16 planes (16 bytes each, `plane` bytes apart) at LDS address d
__device__ __forceinline__ void sp_split8_store(unsigned char* d, const int plane, const float4 lo, const float4 hi) {
  sp_u32x4 p0, p1, p2;
  sp_split8(lo, hi, p0, p1, p2);
  *(sp_lds_u32x4*)(d) = p0;
  *(sp_lds_u32x4*)(d + plane) = p1;
  *(sp_lds_u32x4*)(d + 2 * plane) = p2;
}

// the MFMA A operand of `steps` k steps of one row, raw: per k step the 8 floats at p + 16 s (p: the row + 8 * half of the lane)
__device__ __forceinline__ void sp_load_ksteps(const float* p, float4 (*raw)[2], const int steps) {
#pragma unroll
  for (int s = 0; s < steps; ++s) {
    raw[s][0] = *reinterpret_cast<const float4*>(p + s * 16);
    raw[s][1] = *reinterpret_cast<const float4*>(p + s * 16 + 4);
  }
}

// accumulator register r of a 32 x 32 tile holds row sp_acc_row(r) + 4 * (lane >> 5), column lane & 31
__device__ __forceinline__ constexpr int sp_acc_row(const int r) { return (r & 3) + 8 * (r >> 2); }

// forward epilogue: bias, then the activation (the two common ones without the switch of sbr_act)
__device__ __forceinline__ float sp_bias_act(const float acc, const float bias, const int act) {
  const float v = acc + bias;
  return act == SBR_ACT_NONE ? v : (act == SBR_ACT_RELU ? sbr_relu(v) : sbr_act(v, act));
}

static inline bool sp_al16(const void* p, long ld) { return (((uintptr_t)p) & 15) == 0 && (ld & 3) == 0; }
