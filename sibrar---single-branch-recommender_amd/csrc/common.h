// Shared helpers for the SiBraR HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define SBR_OK 0
#define SBR_ERR_ARG 1
#define SBR_ERR_HIP 2

#define SBR_ACT_NONE 0
#define SBR_ACT_RELU 1
#define SBR_ACT_TANH 2
#define SBR_ACT_SIGMOID 3
#define SBR_ACT_SELU 4

void sbr_set_error(const char* fmt, ...);

#define SBR_REQUIRE(cond, ...)                 \
  do {                                         \
    if (!(cond)) {                             \
      sbr_set_error(__VA_ARGS__);              \
      return SBR_ERR_ARG;                      \
    }                                          \
  } while (0)

#define SBR_CHECK_LAUNCH(name)                                              \
  do {                                                                      \
    hipError_t e__ = hipGetLastError();                                     \
    if (e__ != hipSuccess) {                                                \
      sbr_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return SBR_ERR_HIP;                                                   \
    }                                                                       \
  } while (0)

// selu constants (torch.nn.SELU)
#define SBR_SELU_ALPHA 1.6732632423543772848170429916717f
#define SBR_SELU_SCALE 1.0507009873554804934193349852946f

// torch.relu: a NaN stays a NaN ("x > 0 ? x : 0" — one v_max_f32 — would turn the NaN of an overflowed activation into a clean 0 and
// hide the overflow from every later layer and from the loss)
__device__ __forceinline__ float sbr_relu(float x) { return x < 0.f ? 0.f : x; }

__device__ __forceinline__ float sbr_act(float x, int act) {
  switch (act) {
    case SBR_ACT_RELU: return sbr_relu(x);
    case SBR_ACT_TANH: return tanhf(x);
    case SBR_ACT_SIGMOID: return 1.f / (1.f + expf(-x));
    case SBR_ACT_SELU: return SBR_SELU_SCALE * (x > 0.f ? x : SBR_SELU_ALPHA * (expf(x) - 1.f));
    default: return x;
  }
}

// d act / d pre-activation expressed through the activation OUTPUT y.
__device__ __forceinline__ float sbr_act_grad_from_out(float y, int act) {
  switch (act) {
    case SBR_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case SBR_ACT_TANH: return 1.f - y * y;
    case SBR_ACT_SIGMOID: return y * (1.f - y);
    case SBR_ACT_SELU: return y > 0.f ? SBR_SELU_SCALE : (y + SBR_SELU_SCALE * SBR_SELU_ALPHA);
    default: return 1.f;
  }
}

__device__ __forceinline__ float sbr_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double sbr_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float sbr_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// "This wave's vector-memory operations have been performed" — the wait an agent-scope hand-off needs in front of the workgroup
// barrier that precedes an arrival-counter add (MI355X_MICROARCH.md, Valid forms: every storing wave's s_waitcnt vmcnt(0), the
// barrier, then the counter). Stores and no-return atomics count in vmcnt on gfx950. A workgroup-scope release fence does NOT emit
// this wait (checked in the disassembly: the counter add followed the sum atomics with only lgkmcnt(0) + s_barrier in between), and
// inline asm is invisible to the compiler's wait-count pass, so it cannot be dropped. tools/check_arrival_waits.py greps the built
// kernels for it.
#define SBR_DRAIN_VMEM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

static inline int sbr_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// the byte ranges [a, a + na) and [b, b + nb) meet
static inline bool sbr_overlap(const void* a, long na, const void* b, long nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < (uintptr_t)na : pa - pb < (uintptr_t)nb;
}

// 160 KiB of LDS per CU, all of which one workgroup may use
#define SBR_LDS_MAX 163840

// Raises `kernel`'s dynamic LDS limit to `bytes` where that is still to do. hipFuncSetAttribute configures the CURRENT device's copy of
// a kernel, so `slot` (one static per kernel instantiation) remembers the device it last configured and the limit it set there: the
// attribute is set again only on another device or for more bytes than before (a process that drives several GPUs configures each of
// them; a site whose LDS size depends on run-time arguments keeps the largest limit it has asked for). The slot also remembers the
// kernel, so a slot that is handed another kernel raises that one too instead of skipping it. A failure leaves the slot as it was, so
// the next call tries again.
struct SbrLdsSlot { int dev = -1; int bytes = 0; const void* kernel = nullptr; };
static inline int sbr_raise_lds(const char* who, const void* kernel, SbrLdsSlot* slot, size_t bytes) {
  SBR_REQUIRE(bytes <= SBR_LDS_MAX, "%s: %zu bytes of dynamic LDS asked for, over 160 KiB", who, bytes);
  int dev = -1;
  if (hipGetDevice(&dev) == hipSuccess && dev == slot->dev && kernel == slot->kernel && (int)bytes <= slot->bytes) return SBR_OK;
  if (dev < 0 || hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
    sbr_set_error("%s: cannot raise the dynamic LDS limit to %zu bytes", who, bytes);
    return SBR_ERR_HIP;
  }
  slot->dev = dev;
  slot->bytes = (int)bytes;
  slot->kernel = kernel;
  return SBR_OK;
}

// v is positive and finite (not a NaN, not +inf): pivots, regularisation weights, exponents
__host__ __device__ __forceinline__ bool sbr_pos_finite(float v) { return v > 0.f && v <= 3.402823466e+38f; }

// Host prologue of the kernels that run one workgroup per row and keep a tile of four-byte cells in dynamic LDS (sbr_knn_topk,
// sbr_gram_dense, sbr_p3_walk_dense; sbr_slim_cd_f32 per column, with the whole column as its one tile: tile_cols = cols = m, and its
// static LDS as `fixed`), after the entry point's shape and range checks: `tile_cols` columns per tile, 0 for the default (all
// `cols` of them, clamped to [64, SBR_ROW_TILE_DEFAULT]); `fixed`: the kernel's static LDS bytes. -> the tile width when there is
// something to launch, with the kernel's dynamic LDS limit raised on this device (`slot`: the kernel's slot of sbr_raise_lds);
// 0 for an empty row range (`n_rows` == 0), before the operands are looked at; otherwise minus the error code, with the message set.
#define SBR_ROW_TILE_DEFAULT 32768     // four-byte cells of one tile: 128 KiB
static inline int sbr_row_tile(const char* who, const void* kernel, SbrLdsSlot* slot, int cols, int tile_cols, long fixed, int n_rows,
                               bool operands) {
  if (tile_cols < 0) { sbr_set_error("%s: negative tile_cols %d", who, tile_cols); return -SBR_ERR_ARG; }
  const int tw = tile_cols > 0 ? tile_cols : (cols < SBR_ROW_TILE_DEFAULT ? (cols > 64 ? cols : 64) : SBR_ROW_TILE_DEFAULT);
  const long lds = 4L * tw + fixed;
  if (lds > SBR_LDS_MAX) { sbr_set_error("%s: tile_cols=%d asks for %ld bytes of LDS, over 160 KiB", who, tw, lds); return -SBR_ERR_ARG; }
  if (n_rows == 0) return 0;
  if (!operands) { sbr_set_error("%s: null operand", who); return -SBR_ERR_ARG; }
  const int rc = sbr_raise_lds(who, kernel, slot, (size_t)(SBR_LDS_MAX - fixed));
  return rc ? -rc : tw;
}
