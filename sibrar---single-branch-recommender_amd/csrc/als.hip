// Implicit-feedback ALS (algorithms/mf_algs.py:69-142; Hu, Koren and Volinsky, ICDM 2008): one half-sweep recomputes every row of a factor
// matrix X from the other one, Y [n_y, f], 1 <= f <= 128. With c = alpha * r for an observed entry, c = 1 elsewhere and preference 1 / 0:
//   sbr_als_gram_f32        G = Y^T Y + reg I                                     (shared by every row of the half-sweep)
//   sbr_gram_f32            G = Y^T Y                                             (the same kernels; the truncated SVD's, csrc/svd.hip)
//   sbr_als_solve_rows_f32  A_r = G + sum_{i in S} (alpha r_i - 1) y_i y_i^T,  b_r = sum_{i in S} alpha r_i y_i,  x_r = A_r^-1 b_r
// No float atomics: every element of G, A_r and b_r has one owner and receives its terms in a stated order (include/sibrar_hip.h), the
// factorisation and the two substitutions are fixed sequences, so both entry points give the same bits on every run, for every split of
// the row range, and are valid in deterministic mode. tests/als_ref.py restates the update in float64 and in float32.
#include "block128.h"

#define ALS_TILE 8                    // a thread's register tile of A_r / G: 8 x 8
#define ALS_YS 128                    // floats per staged row of Y (columns [f, 8 * ceil(f / 8)) are staged as zeros)

// ---- G = Y^T Y + reg I ---------------------------------------------------------------------------------------------------------------
#define ALS_G_THREADS 256             // 16 x 16 tiles of 8 x 8
#define ALS_G_SLAB 512                // rows of Y per workgroup: one partial [f, f] per slab, added in slab order by the second launch
#define ALS_G_CHUNK 32                // rows staged at a time

__device__ __forceinline__ void als_load8(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// rows [c0, c0 + nc) of Y (row k of the chunk: source row src(k)) into ys[k][0 .. cols), zeros from column f on
template <class SRC>
__device__ __forceinline__ void als_stage(float* __restrict__ ys, const float* __restrict__ Y, long ldy, int f, int cols, int nc, int threads,
                                          SRC src) {
  for (int e = threadIdx.x; e < nc * cols; e += threads) {
    const int k = e / cols, c = e - k * cols;
    ys[k * ALS_YS + c] = c < f ? Y[src(k) * ldy + c] : 0.f;
  }
}

__global__ __launch_bounds__(ALS_G_THREADS) void als_gram_slab_kernel(const float* __restrict__ Y, long n, long ldy, int f,
                                                                      float* __restrict__ ws) {
#pragma clang fp contract(off)
  __shared__ __align__(16) float ys[ALS_G_CHUNK * ALS_YS];
  const int t = threadIdx.x, i0 = (t >> 4) * ALS_TILE, j0 = (t & 15) * ALS_TILE;
  const int cols = ((f + ALS_TILE - 1) / ALS_TILE) * ALS_TILE;
  const bool active = i0 < f && j0 < f;
  const long lo = (long)blockIdx.x * ALS_G_SLAB, hi = lo + ALS_G_SLAB < n ? lo + ALS_G_SLAB : n;
  float acc[ALS_TILE][ALS_TILE];
#pragma unroll
  for (int a = 0; a < ALS_TILE; ++a)
#pragma unroll
    for (int b = 0; b < ALS_TILE; ++b) acc[a][b] = 0.f;
  for (long c0 = lo; c0 < hi; c0 += ALS_G_CHUNK) {
    const int nc = hi - c0 < ALS_G_CHUNK ? (int)(hi - c0) : ALS_G_CHUNK;
    als_stage(ys, Y, ldy, f, cols, nc, ALS_G_THREADS, [=](int k) { return c0 + k; });
    __syncthreads();
    if (active) {
      for (int k = 0; k < nc; ++k) {
        float yi[ALS_TILE], yj[ALS_TILE];
        als_load8(ys + k * ALS_YS + i0, yi);
        als_load8(ys + k * ALS_YS + j0, yj);
#pragma unroll
        for (int a = 0; a < ALS_TILE; ++a)
#pragma unroll
          for (int b = 0; b < ALS_TILE; ++b) acc[a][b] = fmaf(yi[a], yj[b], acc[a][b]);
      }
    }
    __syncthreads();
  }
  if (!active) return;
  float* out = ws + (long)blockIdx.x * f * f;
#pragma unroll
  for (int a = 0; a < ALS_TILE; ++a)
#pragma unroll
    for (int b = 0; b < ALS_TILE; ++b)
      if (i0 + a < f && j0 + b < f) out[(i0 + a) * f + j0 + b] = acc[a][b];
}

extern "C" long sbr_als_gram_f32_workspace(long n_y, int f) {
  if (n_y <= 0 || f < 1 || f > SBR_BLOCK_MAX) return 0;
  return sbr_slab_ws_bytes(n_y, ALS_G_SLAB, (long)f * f);
}

// the two launches of both Gram entries; `reg` = 0: the plain Gram matrix
static int als_gram_launch(const char* who, const float* Y, long n_y, long ldy, int f, float reg, float* G, long ldg, void* workspace,
                           long workspace_bytes, void* stream) {
  SBR_REQUIRE_WIDTH(who, "f", f);
  SBR_REQUIRE(reg == 0.f || sbr_pos_finite(reg), "%s: reg=%g is not positive and finite", who, (double)reg);
  SBR_REQUIRE_SLAB_ROWS(who, "n_y", n_y, ALS_G_SLAB);
  SBR_TRY(sbr_check_ld(who, "f", f, {{"ldy", ldy}, {"ldg", ldg}}));
  SBR_REQUIRE_OPERANDS(who, G && (Y || n_y == 0));
  SBR_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, sbr_als_gram_f32_workspace(n_y, f), 4);
  const int n_slabs = (int)sbr_slabs(n_y, ALS_G_SLAB);
  if (n_slabs > 0) {
    als_gram_slab_kernel<<<(unsigned)n_slabs, ALS_G_THREADS, 0, (hipStream_t)stream>>>(Y, n_y, ldy, f, (float*)workspace);
    SBR_CHECK_LAUNCH(who);
  }
  // the finishing step: element e = (i, j) of G gets `reg` on the diagonal; sbr_gram_f32 (reg = 0): nothing is added
  sbr_slab_reduce_kernel<<<(unsigned)sbr_cdiv(f * f, 256), 256, 0, (hipStream_t)stream>>>(
      (const float*)workspace, n_slabs, f * f, [=] __device__(int e, float s) {
        const int i = e / f, j = e - i * f;
        G[(long)i * ldg + j] = (i == j && reg != 0.f) ? s + reg : s;
      });
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}

extern "C" int sbr_als_gram_f32(const float* Y, long n_y, long ldy, int f, float reg, float* G, long ldg, void* workspace, long workspace_bytes,
                                void* stream) {
  SBR_REQUIRE(f < 1 || f > SBR_BLOCK_MAX || sbr_pos_finite(reg), "sbr_als_gram_f32: reg=%g is not positive and finite", (double)reg);
  return als_gram_launch("sbr_als_gram_f32", Y, n_y, ldy, f, reg, G, ldg, workspace, workspace_bytes, stream);
}

// G = Y^T Y for the truncated SVD (csrc/svd.hip): the same two launches with nothing added to the diagonal, the same workspace query
extern "C" int sbr_gram_f32(const float* Y, long n_y, long ldy, int f, float* G, long ldg, void* workspace, long workspace_bytes, void* stream) {
  return als_gram_launch("sbr_gram_f32", Y, n_y, ldy, f, 0.f, G, ldg, workspace, workspace_bytes, stream);
}

// ---- x_r = A_r^-1 b_r, one workgroup per row -------------------------------------------------------------------------------------------
#define ALS_THREADS 192               // 136 lower-triangle tiles of 8 x 8 at f = 128; f + 1 <= 129 row owners in the factorisation
#define ALS_CHUNK 24                  // observed entries staged at a time: 12 KiB, so that two workgroups fit one CU's 160 KiB at f = 128
#define ALS_FIXED (ALS_CHUNK * ALS_YS + 32 + 32 + SBR_BLOCK_MAX + SBR_BLOCK_MAX)          // floats of LDS in front of A

static inline size_t als_lds_bytes(int f) { return 4 * ((size_t)ALS_FIXED + sbr_odd_cells(f + 1, f)); }      // A at the odd row stride

// LDS: ys [24][128] the staged rows of Y | wv [24] alpha r - 1 | bw [24] alpha r | diag [128] the pivots' square roots | xs [128] the
// solution | A [(f + 1)][lda]: rows 0 .. f-1 the lower triangle of A_r, then of its Cholesky factor L below the diagonal (the diagonal
// of L is diag; A's own diagonal stays); row f is b_r, then z = L^-1 b_r.
__global__ __launch_bounds__(ALS_THREADS) void als_solve_rows_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                                     const float* __restrict__ data, long r0, const float* __restrict__ Y,
                                                                     long ldy, int f, const float* __restrict__ G, float alpha,
                                                                     float* __restrict__ X, long ldx, int* __restrict__ info) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float als_lds[];
  float* ys = als_lds;
  float* wv = ys + ALS_CHUNK * ALS_YS;
  float* bw = wv + 32;
  float* diag = bw + 32;
  float* xs = diag + SBR_BLOCK_MAX;
  float* A = xs + SBR_BLOCK_MAX;
  const int t = threadIdx.x;
  const long r = r0 + (long)blockIdx.x;
  const long p_beg = indptr[r], p_end = indptr[r + 1];
  float* xr = X + r * ldx;
  if (p_beg >= p_end) {                                             // (the same for the whole workgroup)
    if (t < f) xr[t] = 0.f;
    return;
  }
  const int lda = sbr_odd_ld(f), nb = (f + ALS_TILE - 1) / ALS_TILE, cols = nb * ALS_TILE;
  // ---- A_r and b_r: thread t < nb (nb + 1) / 2 owns the 8 x 8 tile (ti, tj), tj <= ti, in registers; thread t < f owns b[t] ----
  const bool tile = t < nb * (nb + 1) / 2;
  int ti = 0, tj = 0;
  if (tile) {
    int rem = t;
    while (rem > ti) { rem -= ti + 1; ++ti; }
    tj = rem;
  }
  const int i0 = ti * ALS_TILE, j0 = tj * ALS_TILE;
  float acc[ALS_TILE][ALS_TILE];
#pragma unroll
  for (int a = 0; a < ALS_TILE; ++a)
#pragma unroll
    for (int b = 0; b < ALS_TILE; ++b) acc[a][b] = (tile && i0 + a < f && j0 + b < f) ? G[(i0 + a) * f + j0 + b] : 0.f;
  float bacc = 0.f;
  for (long c0 = p_beg; c0 < p_end; c0 += ALS_CHUNK) {
    const int nc = p_end - c0 < ALS_CHUNK ? (int)(p_end - c0) : ALS_CHUNK;
    als_stage(ys, Y, ldy, f, cols, nc, ALS_THREADS, [=](int k) { return (long)indices[c0 + k]; });
    if (t < nc) {
      const float c = alpha * (data ? data[c0 + t] : 1.f);
      bw[t] = c;
      wv[t] = c - 1.f;
    }
    __syncthreads();
    if (tile) {
      for (int k = 0; k < nc; ++k) {
        float yi[ALS_TILE], yj[ALS_TILE];
        als_load8(ys + k * ALS_YS + i0, yi);
        als_load8(ys + k * ALS_YS + j0, yj);
        const float w = wv[k];
#pragma unroll
        for (int a = 0; a < ALS_TILE; ++a) {
          const float wa = w * yi[a];
#pragma unroll
          for (int b = 0; b < ALS_TILE; ++b) acc[a][b] = fmaf(wa, yj[b], acc[a][b]);
        }
      }
    }
    if (t < f)
      for (int k = 0; k < nc; ++k) bacc = fmaf(bw[k], ys[k * ALS_YS + t], bacc);
    __syncthreads();
  }
  if (tile) {
#pragma unroll
    for (int a = 0; a < ALS_TILE; ++a)
#pragma unroll
      for (int b = 0; b < ALS_TILE; ++b)
        if (i0 + a < f && j0 + b < f) A[(i0 + a) * lda + j0 + b] = acc[a][b];
  }
  if (t < f) A[f * lda + t] = bacc;
  __syncthreads();
  // ---- unpivoted Cholesky by columns (block128.h), b_r carried as row f: thread t owns row t ----
  sbr_chol_lds(A, lda, f, f + 1, diag, t, [=](int) { sbr_report_min(info, (int)(1 + r)); });
  // ---- L^T x = z by columns, p descending: thread t owns x[t] ----
  float z = t < f ? A[f * lda + t] : 0.f;
  for (int p = f - 1; p >= 0; --p) {
    if (t == p) xs[p] = z / diag[p];
    __syncthreads();
    if (t < p) z = fmaf(-A[p * lda + t], xs[p], z);
  }
  if (t < f) xr[t] = xs[t];
}

extern "C" int sbr_als_solve_rows_f32(const long* indptr, const int* indices, const float* data, long r0, long r1, const float* Y, long n_y,
                                      long ldy, int f, const float* G, float alpha, float* X, long ldx, int* info, void* stream) {
  SBR_REQUIRE_WIDTH(__func__, "f", f);
  SBR_REQUIRE(sbr_pos_finite(alpha), "%s: alpha=%g is not positive and finite", __func__, (double)alpha);
  SBR_TRY(sbr_check_ld(__func__, "f", f, {{"ldx", ldx}, {"ldy", ldy}}));
  SBR_REQUIRE_ROWS(__func__, r0, r1, 2147483646L);
  SBR_REQUIRE(n_y >= 0, "%s: n_y=%ld is negative", __func__, n_y);
  if (r0 == r1) return SBR_OK;
  SBR_REQUIRE_OPERANDS(__func__, indptr && indices && Y && G && X && info);
  SBR_RAISE_LDS(als_solve_rows_kernel, als_lds_bytes(SBR_BLOCK_MAX));
  als_solve_rows_kernel<<<(unsigned)(r1 - r0), ALS_THREADS, als_lds_bytes(f), (hipStream_t)stream>>>(indptr, indices, data, r0, Y, ldy, f, G, alpha,
                                                                                                 X, ldx, info);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}
