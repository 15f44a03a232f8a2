// The 64 x 64 fp32 tile skeleton that csrc/proto_cos.hip, csrc/anchor_mix.hip and csrc/cluster_affil.hip are built on: a workgroup of 256
// threads owns a tile of 64 rows, a thread a 4 x 4 block of every 64-wide output tile, K-chunks of 32 are staged K-major in LDS, sums
// that cross workgroups are per-workgroup partials folded in workgroup order. DESIGN.md ("The 64 x 64 fp32 tile skeleton") has the
// work-item map, the LDS layout and the determinism rule; what is here is the code, once. Everything is inlined into the including
// kernel: the LDS arrays are the kernel's own, a per-kernel difference is a template argument (a divisor while staging) or a small
// functor (the summand of a column sum, the epilogue of the fold), and the epilogue of a product stays with the caller, which gets the
// accumulators back. The register budget of the including kernels is tight (256 VGPRs from NPT = 2 on): check the compiler's
// kernel-resource-usage remarks after any change here.
//
// Reduction orders are part of the kernels' contract (their outputs are fixed-order, bit for bit): a helper here has ONE order, and
// where two kernels differ (t64_half_sum) the order is a template argument.
#pragma once
#include "common.h"
#include <limits.h>
#include <math.h>
#include <type_traits>

constexpr int T64_T = 64;             // tile edge
constexpr int T64_KC = 32;            // K-chunk
constexpr int T64_LD = T64_T + 4;     // LDS row stride (floats): 16-byte aligned rows, 4-bank shift per k
constexpr int T64_MAX_D = 512;        // widest table row
constexpr int T64_MAX_N = 4 * T64_T;  // most prototypes / anchors / clusters: four register blocks per thread (NPT <= 4)
constexpr int T64_MAX_WG = 1024;      // workgroups of a pass that keeps a partial per workgroup = row splits
constexpr long T64_WS_FLOATS = 16L << 20;   // those partials: at most 64 MiB ...
constexpr int T64_MIN_SPLIT = 64;           // ... but never fewer than 64 splits (32 MiB at the largest partial)
constexpr float T64_EPS = 1e-12f;     // F.normalize's eps

static inline int t64_tiles(long n) { return (int)((n + T64_T - 1) / T64_T); }
// workgroups of a pass over R rows: one per row tile up to the cap, a grid-stride loop over the tiles beyond it
static inline int t64_wgs(long R, int max_wg) { const int t = t64_tiles(R); return t < max_wg ? t : max_wg; }
// row splits (= workgroups) of a pass that writes one partial of `part_floats` floats per workgroup
static inline int t64_splits(long R, long part_floats) {
  long s = T64_WS_FLOATS / part_floats;
  if (s < T64_MIN_SPLIT) s = T64_MIN_SPLIT;
  if (s > T64_MAX_WG) s = T64_MAX_WG;
  const int t = t64_tiles(R);
  return s > t ? t : (int)s;
}

// f(std::integral_constant<int, NPT>) for the number of 64-wide register blocks a thread holds: NPT = tiles(N), N <= T64_MAX_N
template <class F>
static inline void t64_dispatch_npt(int npt, F f) {
  switch (npt) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

// acc[i][c] += sum_k As[k][4 rg + i] * Bs[k][4 cg + c] over one staged K-chunk
__device__ __forceinline__ void t64_mma(const float* __restrict__ As, const float* __restrict__ Bs, int rg, int cg, float (&acc)[4][4]) {
#pragma unroll 8
  for (int k = 0; k < T64_KC; ++k) {
    const float4 a = *reinterpret_cast<const float4*>(As + k * T64_LD + 4 * rg);
    const float4 b = *reinterpret_cast<const float4*>(Bs + k * T64_LD + 4 * cg);
    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(av[i], bv[c], acc[i][c]);
  }
}

__device__ __forceinline__ void t64_zero(float (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;
}

// sum / max over the 16 lanes of a row group (lane bits 0 .. 3); every lane ends with the same bits
__device__ __forceinline__ float t64_row_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float t64_row_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// sum over the 32 lanes sk of a half wave (the pieces of a row that the transposed staging leaves in its 32 lanes). DOWN: xor offsets
// 16, 8, 4, 2, 1 (proto_cos); otherwise 1, 2, 4, 8, 16 (cluster_affil). The two associate differently and each kernel keeps its own.
template <bool DOWN>
__device__ __forceinline__ float t64_half_sum(float v) {
  if (DOWN) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  } else {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, 64);
  }
  return v;
}

// {max(|x|, eps), |x| >= eps ? 1 : 0} of a squared norm: the flag switches the projection term of the gradient off where the clamp of
// the norm is active (torch: clamp_min passes no gradient below its bound). The norms are kept, not their reciprocals, and every
// normalisation is a division: x / |x| is then exactly +-1 for a row of one element, as it is in the reference.
__device__ __forceinline__ void t64_stats(float ss, float& nc, float& flag) {
  const float n = sqrtf(ss);
  nc = fmaxf(n, T64_EPS);
  flag = n >= T64_EPS ? 1.f : 0.f;
}

// stat[p] = t64_stats of row p of X [N, D], one wave per row; out_stat: an optional second destination
static __global__ __launch_bounds__(256) void t64_norm_kernel(const float* __restrict__ X, int N, int D, float* __restrict__ stat,
                                                              float* __restrict__ out_stat) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= N) return;
  const int lane = threadIdx.x & 63;
  float ss = 0.f;
  for (int c = lane; c < D; c += 64) { const float v = X[(long)p * D + c]; ss = fmaf(v, v, ss); }
  ss = sbr_wave_sum(ss);
  float nc, flag;
  t64_stats(ss, nc, flag);
  if (lane == 0) {
    stat[2 * p] = nc; stat[2 * p + 1] = flag;
    if (out_stat) { out_stat[2 * p] = nc; out_stat[2 * p + 1] = flag; }
  }
}

// ---- staging. Transposed: thread (sk = t & 31, sr = t >> 5) writes k = sk of the chunk for the 8 rows sr + 8 q. As stored: thread
// (bc = t & 63, bk = t >> 6) writes column bc for the 8 k = bk + 4 q. Everything outside the operand is zero-filled.

// the table rows of the 8 tile rows this thread stages (rows: the lookup, or NULL), NULL past R
__device__ __forceinline__ void t64_row_ptrs(const float* (&rp)[8], const float* __restrict__ W, long ldw, const int* __restrict__ rows,
                                             long j0, long R, int sr) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const long j = j0 + sr + 8 * q;
    rp[q] = j < R ? W + (long)(rows ? rows[j] : j) * ldw : nullptr;
  }
}
// a transposed chunk of looked-up / plain rows: Xs[d - d0][row]
__device__ __forceinline__ void t64_stage_rows_t(float* __restrict__ Xs, const float* const (&rp)[8], int d, int D, int sk, int sr) {
#pragma unroll
  for (int q = 0; q < 8; ++q) Xs[sk * T64_LD + sr + 8 * q] = (rp[q] && d < D) ? rp[q][d] : 0.f;
}
// the same, and where `sq`, the squares are added to ss[q] on the way in
__device__ __forceinline__ void t64_stage_rows_t(float* __restrict__ Xs, const float* const (&rp)[8], int d, int D, int sk, int sr,
                                                 float (&ss)[8], bool sq) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float v = (rp[q] && d < D) ? rp[q][d] : 0.f;
    Xs[sk * T64_LD + sr + 8 * q] = v;
    if (sq) ss[q] = fmaf(v, v, ss[q]);
  }
}
// a transposed chunk of the tile pt of the operand matrix A [N, D]: Bs[d - d0][n - 64 pt]
__device__ __forceinline__ void t64_stage_tile_t(float* __restrict__ Bs, const float* __restrict__ A, int pt, int N, int d, int D, int sk,
                                                 int sr) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int n = pt * T64_T + sr + 8 * q;
    Bs[sk * T64_LD + sr + 8 * q] = (n < N && d < D) ? A[(long)n * D + d] : 0.f;
  }
}
// 32 rows n0 .. n0 + 31 of A [N, D] as stored: Bs[n - n0][d - 64 dt]; NORM: each divided by its norm stat[2 n]
template <bool NORM>
__device__ __forceinline__ void t64_stage_chunk(float* __restrict__ Bs, const float* __restrict__ A, const float* __restrict__ stat, int n0,
                                                int N, int dt, int D, int bc, int bk) {
  const int d = dt * T64_T + bc;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int k = bk + 4 * q, n = n0 + k;
    float v = 0.f;
    if (n < N && d < D) v = NORM ? A[(long)n * D + d] / stat[2 * n] : A[(long)n * D + d];
    Bs[k * T64_LD + bc] = v;
  }
}
// the half `half` (32 columns) of a thread-held [64 rows, 64 columns] block, transposed: As[column - 32 half][row]
__device__ __forceinline__ void t64_stage_regs_t(float* __restrict__ As, const float (&v)[4][4], int half, int rg, int cg) {
  if ((cg >> 3) == half) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<float4*>(As + (4 * (cg & 7) + c) * T64_LD + 4 * rg) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
  }
}
// the half `half` (32 rows) of a thread-held block as it is: As[row - 32 half][column]
__device__ __forceinline__ void t64_stage_regs(float* __restrict__ As, const float (&v)[4][4], int half, int rg, int cg) {
  if ((rg >> 3) == half) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<float4*>(As + (4 * (rg & 7) + i) * T64_LD + 4 * cg) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
  }
}

// ---- products of the thread-held [64, N] block set

// acc[row, d] = sum_n v[row, n] A[n, d] for the tile dtile of D: v is the thread-held block set (zero for n >= N), A [N, D]
template <int NPT>
__device__ __forceinline__ void t64_regs_times(float* __restrict__ As, float* __restrict__ Bs, const float (&v)[NPT][4][4],
                                               const float* __restrict__ A, int N, int D, int dtile, int t, float (&acc)[4][4]) {
  const int cg = t & 15, rg = t >> 4, bc = t & 63, bk = t >> 6;
  t64_zero(acc);
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int n0 = pt * T64_T + half * T64_KC;
      if (n0 < N) {                                     // the same for every thread
        t64_stage_regs_t(As, v[pt], half, rg, cg);
        t64_stage_chunk<false>(Bs, A, nullptr, n0, N, dtile, D, bc, bk);
        __syncthreads();
        t64_mma(As, Bs, rg, cg, acc);
        __syncthreads();
      }
    }
  }
}
// out[j0 + row, 64 dtile + col] = acc for the rows below R and the columns below D
__device__ __forceinline__ void t64_store_rows(float* __restrict__ out, long ldo, const float (&acc)[4][4], long j0, long R, int dtile, int D,
                                               int t) {
  const int cg = t & 15, rg = t >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long j = j0 + 4 * rg + i;
    if (j >= R) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int d = dtile * T64_T + 4 * cg + c;
      if (d < D) out[j * ldo + d] = acc[i][c];
    }
  }
}

// acc[n, d] += sum_j v[j - j0, n] X[row(j), d] over the 32 rows of the half `half` of the tile, for the tile dtile of D: v is one
// thread-held block, row(j) = rows[j] or j. Rows past R and columns past D are zero.
__device__ __forceinline__ void t64_regs_t_times(float* __restrict__ As, float* __restrict__ Bs, const float (&v)[4][4], int half,
                                                 const float* __restrict__ X, long ldx, const int* __restrict__ rows, long j0, long R,
                                                 int dtile, int D, int t, float (&acc)[4][4]) {
  const int cg = t & 15, rg = t >> 4, bc = t & 63, bk = t >> 6;
  const int d = dtile * T64_T + bc;
  t64_stage_regs(As, v, half, rg, cg);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int rl = bk + 4 * q;
    const long j = j0 + half * T64_KC + rl;
    Bs[rl * T64_LD + bc] = (j < R && d < D) ? X[(long)(rows ? rows[j] : j) * ldx + d] : 0.f;
  }
  __syncthreads();
  t64_mma(As, Bs, rg, cg, acc);
  __syncthreads();
}
// this tile's block (pt, dtile) of the workgroup's own partial [N, D]: stored for the workgroup's first tile, added after it (the same
// thread owns the element in every tile)
__device__ __forceinline__ void t64_part_add(float* my_part, const float (&acc)[4][4], int pt, int N, int dtile, int D, int t,
                                             bool first) {
  const int cg = t & 15, rg = t >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = pt * T64_T + 4 * rg + i;
    if (n >= N) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int dd = dtile * T64_T + 4 * cg + c;
      if (dd < D) {
        float* p = my_part + (long)n * D + dd;
        *p = first ? acc[i][c] : *p + acc[i][c];
      }
    }
  }
}

// s_col[n] += the sum over this tile's rows of column n, n < N: f(pt, c) is the thread's own share (its four rows of column 64 pt +
// 4 cg + c), then the row groups of a wave (lane bits 4, 5), then the four waves through s_wc as (w0 + w1) + (w2 + w3)
template <int NPT, class Acc, class F>
__device__ __forceinline__ void t64_col_sums(float (&s_wc)[4][T64_T], Acc* __restrict__ s_col, int N, int t, F f) {
  const int cg = t & 15, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float cs = f(pt, c);
      cs += __shfl_xor(cs, 16, 64);
      cs += __shfl_xor(cs, 32, 64);
      if (lane < 16) s_wc[wave][4 * cg + c] = cs;
    }
    __syncthreads();
    if (t < T64_T && pt * T64_T + t < N) s_col[pt * T64_T + t] += (Acc)((s_wc[0][t] + s_wc[1][t]) + (s_wc[2][t] + s_wc[3][t]));
    __syncthreads();
  }
}

// out[n, d] = epi(e, n, sum over the splits of part[split][n, d], sum over the splits of part_cs[split][n]): both sums in split order,
// in double, rounded to fp32 once. Epi::kColumnSums false: no second sum (part_cs is not read). epi is the caller's own expression (a plain copy, or one of the two
// normalisation-gradient forms, which differ in their rounding).
template <class Epi>
static __global__ __launch_bounds__(256) void t64_fold_kernel(const float* __restrict__ part, const float* __restrict__ part_cs, int n_split,
                                                              int N, int D, Epi epi, float* __restrict__ out) {
  const long e = blockIdx.x * 256L + threadIdx.x, ND = (long)N * D;
  if (e >= ND) return;
  const int n = (int)(e / D);
  double s = 0.0, cs = 0.0;
#pragma unroll 4
  for (int sp = 0; sp < n_split; ++sp) {
    s += (double)part[sp * ND + e];
    if (Epi::kColumnSums) cs += (double)part_cs[(long)sp * N + n];
  }
  out[e] = epi(e, n, (float)s, (float)cs);
}
