// The multinomial log-likelihood of Mult-VAE / Mult-DAE (Liang et al., WWW 2018) for a [B, n_items] logit matrix against the users' rows
// of a binary CSR matrix, with its gradient. One entry:
//   sbr_multinomial_nll_f32  row_loss[b] = n * lse(z) - sum of z at the row's items;  dlogits[b][j] = gs * (n * exp(z_j - lse) - [j in row])
// Two passes over a row. Pass 1 is an online softmax: a thread keeps a running (max, sum of exponentials relative to it) over the
// four-float chunks it owns and the pairs are merged across the row's threads in a fixed tree, so the logits are read once for both
// the maximum and the sum. Pass 2 writes the dense part of the gradient; the row's owner (a wave or a workgroup) then subtracts gs at
// the row's items behind its own dense write. Chunk c of a row (elements 4c .. 4c + 3) belongs to thread c % T of the T threads that
// own the row whether it is loaded as one float4 or as four floats, so the order of every floating-point operation depends on n_items
// alone: not on the alignment of the operands, on B, on b, on the run or on the other rows. No atomics.
// include/sibrar_hip.h states the definition; tests/multvae_ref.py derives the error bound from the geometry below.
#include "common.h"

#define MN_THREADS 256
#define MN_WAVES (MN_THREADS / 64)
#define MN_WAVE_MAX 1024               // rows up to here: a wave per row, MN_WAVES rows per workgroup
#define MN_STAGE_MAX 12288             // rows up to here: a workgroup per row, the row kept in LDS between the passes (48 KiB: 3 workgroups per CU)
#define MN_GRID_MAX (1 << 20)          // workgroups of a launch; the rows beyond are taken by a grid-stride loop

struct MnPair { float m, s; };         // s = sum of expf(z - m) over the elements seen so far; nothing seen: (-inf, 0)

// expf(from - to) for from <= to, and exactly 1 where they are equal (also for -inf, -inf: a thread that owns no element)
__device__ __forceinline__ float mn_rescale(float from, float to) { return from == to ? 1.f : expf(from - to); }

__device__ __forceinline__ MnPair mn_merge(MnPair a, MnPair b) {
#pragma clang fp contract(off)                                     // a * x + b * y without an fma: the same bits on both sides of a butterfly
  MnPair r;
  r.m = fmaxf(a.m, b.m);
  const float sa = a.s * mn_rescale(a.m, r.m), sb = b.s * mn_rescale(b.m, r.m);
  r.s = sa + sb;
  return r;
}

// chunk c of a row of n_items floats; the elements past the row's end come back as -inf (they add expf(-inf) = 0 to a sum)
template <bool VEC>
__device__ __forceinline__ void mn_load4(const float* row, int c, int n_items, float* v) {
  if (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(row + 4L * c);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = 4L * c + k < n_items ? row[4L * c + k] : -INFINITY;
  }
}

template <bool VEC>
__device__ __forceinline__ void mn_store4(float* row, int c, int n_items, const float* v) {
  if (VEC) {
    *reinterpret_cast<float4*>(row + 4L * c) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4L * c + k < n_items) row[4L * c + k] = v[k];
  }
}

// One row by T threads (T = 64: a wave, no barrier; T = MN_THREADS: the workgroup). t: the thread's index among the T; `stage`: the
// row's image in LDS (STAGE) where a thread keeps the chunks it owns between the passes; `red`: MN_WAVES pairs and MN_WAVES floats.
template <bool VEC, int T, bool STAGE>
__device__ __forceinline__ void mn_row(const long* __restrict__ indptr, const int* __restrict__ indices, long u, int n_items,
                                       const float* zrow, float* drow, float gs, float* row_loss, float* row_lse, long b, int t,
                                       float* stage, float* red) {
#pragma clang fp contract(off)
  const int chunks = (n_items + 3) >> 2;
  const long beg = indptr[u], end = indptr[u + 1];
  // ---- pass 1: the thread's running (max, sum) over its chunks in ascending order, and its share of the positives -------------
  MnPair p = {-INFINITY, 0.f};
  for (int c = t; c < chunks; c += T) {
    float v[4];
    mn_load4<VEC>(zrow, c, n_items, v);
    if (STAGE) *reinterpret_cast<float4*>(stage + 4 * c) = make_float4(v[0], v[1], v[2], v[3]);
    const float m = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), p.m);
    float s = p.s * mn_rescale(p.m, m);
#pragma unroll
    for (int k = 0; k < 4; ++k) s = s + expf(v[k] - m);
    p.m = m;
    p.s = s;
  }
  float pos = 0.f;
  for (long e = beg + t; e < end; e += T) {
    const int i = indices[e];
    if ((unsigned)i < (unsigned)n_items) pos = pos + zrow[i];       // (an index outside the row is the caller's error: nothing is read there)
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    MnPair q;
    q.m = __shfl_xor(p.m, o, 64);
    q.s = __shfl_xor(p.s, o, 64);
    p = mn_merge(p, q);
    pos = pos + __shfl_xor(pos, o, 64);
  }
  if (T > 64) {
    MnPair* rp = reinterpret_cast<MnPair*>(red);
    float* rs = red + 2 * MN_WAVES;
    if ((t & 63) == 0) {
      rp[t >> 6] = p;
      rs[t >> 6] = pos;
    }
    __syncthreads();
    p = rp[0];
    pos = rs[0];
#pragma unroll
    for (int w = 1; w < MN_WAVES; ++w) {
      p = mn_merge(p, rp[w]);
      pos = pos + rs[w];
    }
  }
  const float lse = p.m + logf(p.s);
  const long n = end - beg;
  const float fn = (float)n;
  if (t == 0) {
    row_loss[b] = n > 0 ? fn * lse - pos : 0.f;
    if (row_lse) row_lse[b] = lse;
  }
  if (!drow) return;
  // ---- pass 2: the dense part of the gradient, every thread over the chunks it read in pass 1 ---------------------------------
  for (int c = t; c < chunks; c += T) {
    float v[4], g[4];
    if (STAGE) {
      const float4 q = *reinterpret_cast<const float4*>(stage + 4 * c);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      mn_load4<VEC>(zrow, c, n_items, v);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = n > 0 ? gs * (fn * expf(v[k] - lse)) : 0.f;
    mn_store4<VEC>(drow, c, n_items, g);
  }
  if (n == 0) return;
  // ---- the positives: one owner per element (indices are unique), behind the owner's dense write of the row ------------------
  SBR_DRAIN_VMEM();
  if (T > 64) __syncthreads();
  for (long e = beg + t; e < end; e += T) {
    const int i = indices[e];
    if ((unsigned)i < (unsigned)n_items) drow[i] = drow[i] - gs;
  }
}

template <bool VEC>
__global__ __launch_bounds__(MN_THREADS) void mn_wave_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                             const long* __restrict__ rows, long B, int n_items, const float* logits,
                                                             float* dlogits, float gs, float* row_loss, float* row_lse) {
  const int lane = threadIdx.x & 63;
  for (long b = (long)blockIdx.x * MN_WAVES + (threadIdx.x >> 6); b < B; b += (long)gridDim.x * MN_WAVES)
    mn_row<VEC, 64, false>(indptr, indices, rows[b], n_items, logits + b * n_items, dlogits ? dlogits + b * n_items : nullptr, gs, row_loss,
                           row_lse, b, lane, nullptr, nullptr);
}

template <bool VEC, bool STAGE>
__global__ __launch_bounds__(MN_THREADS) void mn_block_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                              const long* __restrict__ rows, long B, int n_items, const float* logits,
                                                              float* dlogits, float gs, float* row_loss, float* row_lse) {
  extern __shared__ __align__(16) float mn_stage[];
  __shared__ float red[3 * MN_WAVES];
  for (long b = blockIdx.x; b < B; b += gridDim.x) {
    mn_row<VEC, MN_THREADS, STAGE>(indptr, indices, rows[b], n_items, logits + b * n_items, dlogits ? dlogits + b * n_items : nullptr, gs,
                                   row_loss, row_lse, b, threadIdx.x, mn_stage, red);
    __syncthreads();                                               // `red` is free for the next row
  }
}

extern "C" int sbr_multinomial_nll_f32(const long* indptr, const int* indices, const long* rows, long B, int n_items, const float* logits,
                                       float* dlogits, float grad_scale, float* row_loss, float* row_lse, void* stream) {
  SBR_REQUIRE(n_items >= 1, "sbr_multinomial_nll_f32: n_items=%d is not positive", n_items);
  SBR_REQUIRE(B >= 0, "sbr_multinomial_nll_f32: B=%ld is negative", B);
  SBR_REQUIRE(indptr && rows && logits && row_loss, "sbr_multinomial_nll_f32: null operand (indptr, rows, logits or row_loss)");
  const long mat = 4L * B * n_items, vec = 4L * B;
  SBR_REQUIRE(!(dlogits && dlogits != logits && sbr_overlap(logits, mat, dlogits, mat)), "sbr_multinomial_nll_f32: dlogits overlaps logits "
              "in part: it is logits itself (in place) or a disjoint matrix");
  SBR_REQUIRE(!sbr_overlap(row_loss, vec, logits, mat) && !(dlogits && sbr_overlap(row_loss, vec, dlogits, mat)),
              "sbr_multinomial_nll_f32: row_loss overlaps logits or dlogits");
  SBR_REQUIRE(!(row_lse && (sbr_overlap(row_lse, vec, logits, mat) || (dlogits && sbr_overlap(row_lse, vec, dlogits, mat)))),
              "sbr_multinomial_nll_f32: row_lse overlaps logits or dlogits");
  SBR_REQUIRE(!(row_lse && sbr_overlap(row_lse, vec, row_loss, vec)), "sbr_multinomial_nll_f32: row_lse overlaps row_loss");
  if (B == 0) return SBR_OK;
  // float4 where every row of both matrices starts on a 16-byte boundary, four floats per chunk otherwise: the same chunks, the same order
  const bool v4 = n_items % 4 == 0 && ((uintptr_t)logits | (uintptr_t)dlogits) % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
#define MN_ARGS indptr, indices, rows, B, n_items, logits, dlogits, grad_scale, row_loss, row_lse
  if (n_items <= MN_WAVE_MAX) {
    const long blocks = (B + MN_WAVES - 1) / MN_WAVES;
    const unsigned grid = (unsigned)(blocks < MN_GRID_MAX ? blocks : MN_GRID_MAX);
    if (v4) mn_wave_kernel<true><<<grid, MN_THREADS, 0, st>>>(MN_ARGS); else mn_wave_kernel<false><<<grid, MN_THREADS, 0, st>>>(MN_ARGS);
  } else {
    const unsigned grid = (unsigned)(B < MN_GRID_MAX ? B : MN_GRID_MAX);
    if (n_items <= MN_STAGE_MAX) {
      const size_t lds = 16 * (size_t)((n_items + 3) / 4);
      if (v4) mn_block_kernel<true, true><<<grid, MN_THREADS, lds, st>>>(MN_ARGS); else mn_block_kernel<false, true><<<grid, MN_THREADS, lds, st>>>(MN_ARGS);
    } else {
      if (v4) mn_block_kernel<true, false><<<grid, MN_THREADS, 0, st>>>(MN_ARGS); else mn_block_kernel<false, false><<<grid, MN_THREADS, 0, st>>>(MN_ARGS);
    }
  }
#undef MN_ARGS
  SBR_CHECK_LAUNCH("sbr_multinomial_nll_f32");
  return SBR_OK;
}
