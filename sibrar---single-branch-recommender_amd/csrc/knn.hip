// Neighbourhood models on 0/1 interaction data (algorithms/knn_algs.py: UserKNN, ItemKNN).
//   sbr_knn_topk            the k most similar rows of every row of a binary CSR matrix: co-occurrence counts, similarity value and
//                           top-k selection of one row inside one workgroup (utilities/similarities.py:18-130)
//   sbr_csr_rows_times_csr  dense rows of a CSR x CSR product: both predictions (knn_algs.py:96, :116)
// Nothing of size n x n or block x n exists: a workgroup owns one row of the similarity matrix from the first count to the sorted list.
// No float atomics anywhere: the counts are integers (LDS integer atomics: exact, order-free), every float has one owner and a fixed
// operation order, so both entries give the same bits on every run and are valid in deterministic mode.
#include "common.h"
#include "csr_walk.h"
#include "cooc_topk.h"

#define KNN_THREADS 1024
#define KNN_WAVES (KNN_THREADS / 64)
#define KNN_K_MAX 256                // the limit of sbr_topk_rows
#define KNN_M_MAX (1 << 24)          // counts and row sizes are converted to fp32 exactly

#define KNN_COSINE 0
#define KNN_JACCARD 1
#define KNN_ASYMMETRIC_COSINE 2
#define KNN_SORENSEN_DICE 3
#define KNN_TVERSKY 4

// The similarity of two rows with c > 0 common features, ni and nj features each. Every operation is one correctly rounded fp32
// operation in exactly this order (no contraction of a product and a sum into an fma); the integer sums are exact and are converted
// once. include/sibrar_hip.h states the same order, tests/knn_ref.py derives its bound from it.
__device__ __forceinline__ float knn_value(int sim, unsigned int c, int ni, int nj, float alpha, float beta, float shrinkage) {
#pragma clang fp contract(off)
  const float cf = (float)c;
  float v;
  switch (sim) {
    case KNN_COSINE: {
      const float d = sqrtf((float)ni) * sqrtf((float)nj);
      v = cf / d;
      break;
    }
    case KNN_JACCARD:
      v = cf / (float)(ni + nj - (int)c);
      break;
    case KNN_ASYMMETRIC_COSINE: {
      const float oma = 1.f - alpha;
      const float d = powf((float)ni, alpha) * powf((float)nj, oma);
      v = cf / d;
      break;
    }
    case KNN_SORENSEN_DICE:
      v = (2.f * cf) / (float)(ni + nj);
      break;
    default: {    // KNN_TVERSKY
      const float a = alpha * (float)(ni - (int)c), b = beta * (float)(nj - (int)c);
      const float d = (cf + a) + b;
      v = cf / d;
      break;
    }
  }
  const float s = cf / (cf + shrinkage);
  return v * s;
}

// One workgroup per row i of X. The entity columns are covered by tiles of `tw` u32 counters in LDS. Per tile:
//   count    wave w takes the features w, w + 16, ... of row i and walks X^T's row of each (entered at the tile's start by a lower
//            bound), adding 1 to cnt[j - t0]                                                             (sbr_cooc_count_tile, csr_walk.h);
//   value    every counter c > 0 with j != i is replaced in place by the bits of its similarity (> 0, so the bits order like the
//            values), everything else by 0;
//   select   the k largest composites among the list carried from the earlier tiles and this tile's entries
//                                                                                                 (sbr_topk_select_tile, cooc_topk.h).
// After the last tile the list is sorted (bitonic) and written with its length and the (-1, 0) padding (sbr_topk_sort_write).
__global__ __launch_bounds__(KNN_THREADS) void knn_topk_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                                const long* __restrict__ t_indptr, const int* __restrict__ t_indices,
                                                                int n, int r0, int sim, float alpha, float beta, float shrinkage, int k,
                                                                int kpad, int tw, int* __restrict__ nbr_idx, float* __restrict__ nbr_val,
                                                                int* __restrict__ nbr_len) {
  extern __shared__ unsigned int cnt[];
  __shared__ SbrTopkLds<KNN_K_MAX> sel;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i = r0 + (int)blockIdx.x;
  const long f_beg = indptr[i], f_end = indptr[i + 1];
  const int ni = (int)(f_end - f_beg);
  int cur = 0;                 // sel.lists[cur]: the list carried so far, n_list entries, unsorted
  unsigned int n_list = 0;

  for (int t0 = 0; t0 < n && ni > 0; t0 += tw) {
    const int t1 = t0 + tw < n ? t0 + tw : n, width = t1 - t0;
    for (int x = t; x < width; x += KNN_THREADS) cnt[x] = 0u;
    __syncthreads();
    // ---- count
    sbr_cooc_count_tile(indices, f_beg, f_end, t_indptr, t_indices, t0, width, w, KNN_WAVES, lane, cnt);
    __syncthreads();
    // ---- value, in place
    for (int x = t; x < width; x += KNN_THREADS) {
      const unsigned int c = cnt[x];
      const int j = t0 + x;
      if (c != 0u) cnt[x] = j == i ? 0u : __float_as_uint(knn_value(sim, c, ni, (int)(indptr[j + 1] - indptr[j]), alpha, beta, shrinkage));
    }
    // ---- select
    sbr_topk_select_tile<KNN_THREADS>(sel, cnt, width, t0, k, cur, n_list);
  }
  sbr_topk_sort_write<KNN_THREADS>(sel, cur, n_list, k, kpad, i, nbr_idx, nbr_val, nbr_len);
}

extern "C" int sbr_knn_topk(const long* indptr, const int* indices, const long* t_indptr, const int* t_indices, int n, int m, int r0,
                            int r1, int sim, float alpha, float beta, float shrinkage, int k, int tile_cols, int* nbr_idx,
                            float* nbr_val, int* nbr_len, void* stream) {
  SBR_REQUIRE(k >= 1 && k <= KNN_K_MAX, "sbr_knn_topk: k=%d outside [1, %d]", k, KNN_K_MAX);
  SBR_REQUIRE(sim >= KNN_COSINE && sim <= KNN_TVERSKY, "sbr_knn_topk: unknown similarity code %d", sim);
  SBR_REQUIRE(shrinkage >= 0.f, "sbr_knn_topk: negative shrinkage %g", (double)shrinkage);
  SBR_REQUIRE(alpha >= 0.f && beta >= 0.f, "sbr_knn_topk: negative alpha / beta (%g, %g)", (double)alpha, (double)beta);
  SBR_REQUIRE(n >= 0 && m >= 0 && m <= KNN_M_MAX, "sbr_knn_topk: shape [%d, %d] outside [0, 2^31) x [0, 2^24]", n, m);
  SBR_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= n, "sbr_knn_topk: row range [%d, %d) outside [0, %d]", r0, r1, n);
  const long fixed = (long)sizeof(SbrTopkLds<KNN_K_MAX>) + 40;   // the kernel's static LDS: two lists, the histogram, the scalars
  static SbrLdsSlot lds_slot;
  const int tw = sbr_row_tile("sbr_knn_topk", (const void*)knn_topk_kernel, &lds_slot, n, tile_cols, fixed, r1 - r0,
                              indptr && indices && t_indptr && t_indices && nbr_idx && nbr_val && nbr_len);
  if (tw <= 0) return -tw;
  int kpad = 2;
  while (kpad < k) kpad <<= 1;
  knn_topk_kernel<<<(unsigned)(r1 - r0), KNN_THREADS, 4 * (size_t)tw, (hipStream_t)stream>>>(indptr, indices, t_indptr, t_indices, n, r0, sim,
                                                                                      alpha, beta, shrinkage, k, kpad, tw, nbr_idx, nbr_val, nbr_len);
  SBR_CHECK_LAUNCH("sbr_knn_topk");
  return SBR_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// out[b, c] = sum over the entries p of X's row rows[b], in ascending column of X, of x[p] * Y[col(p), c]      (0 <= c < n_cols)
// A wave owns (row b, `sub` consecutive columns) with its accumulators in its own slice of LDS; four waves share a workgroup and
// nothing else. The wave loads 64 entries of X's row at a time (column, value, the bounds of Y's row) and then takes them one after
// the other: its lanes cover Y's row, whose columns are distinct, so no two lanes meet on an accumulator, and an accumulator sees
// its terms in the order of X's entries: acc = fmaf(x, y, acc), one rounding per term. Short rows of Y are scanned from their start
// (two loads cover 128 entries), longer ones are entered at the slice's first column by a lower bound.
// ---------------------------------------------------------------------------------------------------------------
#define CXC_WAVES 4
#define CXC_TILE_DEFAULT 8192        // columns per workgroup: 32 KiB of accumulators, five workgroups (20 waves) per CU
#define CXC_SCAN_MAX 128

__global__ __launch_bounds__(64 * CXC_WAVES) void csr_rows_times_csr_kernel(const long* __restrict__ x_indptr, const int* __restrict__ x_indices,
                                                                            const float* __restrict__ x_data, const long* __restrict__ rows,
                                                                            const long* __restrict__ y_indptr, const int* __restrict__ y_indices,
                                                                            const float* __restrict__ y_data, int n_cols, int sub,
                                                                            long b0, float* __restrict__ out, long ld) {
  extern __shared__ float acc_all[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long c_beg = ((long)blockIdx.x * CXC_WAVES + w) * sub;
  if (c_beg >= n_cols) return;                              // (no workgroup barrier below: the waves are independent)
  const int cb = (int)c_beg, width = cb + sub < n_cols ? sub : n_cols - cb;
  float* acc = acc_all + (long)w * sub;
  for (int x = lane; x < width; x += 64) acc[x] = 0.f;
  const long b = b0 + blockIdx.y;
  const long r = rows ? rows[b] : b;
  const long p_end = x_indptr[r + 1];
  for (long p0 = x_indptr[r]; p0 < p_end; p0 += 64) {
    const int n_e = p_end - p0 < 64 ? (int)(p_end - p0) : 64;
    int my_beg = 0, my_len = 0;
    long my_base = 0;
    float my_x = 0.f;
    if (lane < n_e) {
      const int j = x_indices[p0 + lane];
      my_x = x_data ? x_data[p0 + lane] : 1.f;
      my_base = y_indptr[j];
      my_len = (int)(y_indptr[j + 1] - my_base);
      if (my_len > CXC_SCAN_MAX) my_beg = sbr_csr_lower_bound(y_indices + my_base, 0, my_len, cb);
    }
    for (int e = 0; e < n_e; ++e) {
      const float xv = __shfl(my_x, e, 64);
      const long base = __shfl(my_base, e, 64);
      const int len = __shfl(my_len, e, 64);
      for (int q = __shfl(my_beg, e, 64) + lane; q < len; q += 64) {
        const unsigned int x = (unsigned int)(y_indices[base + q] - cb);
        if ((int)x >= width) break;                         // sorted: the rest of Y's row belongs to later slices
        if (x < (unsigned int)width) acc[x] = fmaf(xv, y_data ? y_data[base + q] : 1.f, acc[x]);
      }
      // the next entry may name the same accumulator from another lane: keep the LDS accesses of two entries in program order
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float* o = out + b * ld + cb;
  for (int x = lane; x < width; x += 64) o[x] = acc[x];
}

extern "C" int sbr_csr_rows_times_csr(const long* x_indptr, const int* x_indices, const float* x_data, const long* rows, long B,
                                      const long* y_indptr, const int* y_indices, const float* y_data, int n_cols, int tile_cols,
                                      float* out, long ld, void* stream) {
  SBR_REQUIRE(B >= 0 && B <= 65535L * 65535L && n_cols >= 0 && ld >= n_cols, "sbr_csr_rows_times_csr: bad shape (B=%ld, n_cols=%d, ld=%ld)", B,
              n_cols, ld);
  SBR_REQUIRE(tile_cols >= 0, "sbr_csr_rows_times_csr: negative tile_cols %d", tile_cols);
  if (B == 0 || n_cols == 0) return SBR_OK;
  SBR_REQUIRE(x_indptr && y_indptr && out, "sbr_csr_rows_times_csr: null operand");
  int tile = tile_cols > 0 ? tile_cols : (n_cols < CXC_TILE_DEFAULT ? n_cols : CXC_TILE_DEFAULT);
  const int sub = (int)((tile + CXC_WAVES - 1) / CXC_WAVES);
  const long lds = 4L * sub * CXC_WAVES;
  SBR_REQUIRE(lds <= 65536, "sbr_csr_rows_times_csr: tile_cols=%d asks for %ld bytes of LDS, over 64 KiB", tile_cols, lds);
  const long per_wg = (long)sub * CXC_WAVES;
  const unsigned gx = (unsigned)((n_cols + per_wg - 1) / per_wg);
  // the rows go to gridDim.y (<= 65535): longer batches in slabs
  for (long b0 = 0; b0 < B; b0 += 65535) {
    const unsigned gy = (unsigned)(B - b0 < 65535 ? B - b0 : 65535);
    csr_rows_times_csr_kernel<<<dim3(gx, gy), 64 * CXC_WAVES, (size_t)lds, (hipStream_t)stream>>>(
        x_indptr, x_indices, x_data, rows, y_indptr, y_indices, y_data, n_cols, sub, b0, out, ld);
    SBR_CHECK_LAUNCH("sbr_csr_rows_times_csr");
  }
  return SBR_OK;
}
