// Neighbourhood model on dense item features (algorithms/knn_algs.py:121-140 ItemFeatureKNN; utilities/similarities.py:18-61, :86-93).
//   sbr_row_norms_f32    norm_i = sqrtf(sum_k F[i,k]^2), the sum as an fmaf chain over k ascending (the bits of dot_ii below)
//   sbr_dense_knn_topk   the k most similar rows of every row of a dense fp32 matrix: the n x n x d product on the fp32 matrix pipe,
//                        cosine value, candidate filter and top-k selection inside the workgroup that owns the query rows
// Nothing of size n x n or rows x n exists and there is no workspace: a workgroup owns DK_ROWS query rows from the first product to the
// sorted lists. v_mfma_f32_32x32x2_f32 is bit for bit acc = fmaf(a_k, b_k, acc) over k ascending (csrc/ease.hip relies on the same), and
// fmaf(a, b, .) = fmaf(b, a, .), so dot_ij and dot_ji carry the same bits whatever tile the pair falls in. No float atomics: the
// appends to a row's candidate buffer take their slots by integer LDS atomics, and the composites (key << 32 | ~index) are distinct, so
// the selected set and the sorted list do not depend on the slot order. The same bits on every run and for every split of the rows.
#include "common.h"
#include "score_topk_common.h"

#define DK_THREADS 256
#define DK_WAVES (DK_THREADS / 64)
#define DK_ROWS 32                   // query rows of a workgroup: one 32-row MFMA tile, shared by the four waves
#define DK_COLS (32 * DK_WAVES)      // candidate rows of a column tile: 32 per wave
#define DK_KC 32                     // k-chunk staged through LDS
#define DK_LDP (DK_KC + 1)           // row stride of the staged chunks: the 32 rows an operand read names fall into distinct banks
#define DK_K_MAX 256
#define DK_D_MAX 8192
#define DK_EPL_MAX ((DK_K_MAX + DK_COLS) / 64)       // buffer entries per lane of the wave that reduces a row

// The similarity of two distinct rows with dot != 0: one correctly rounded fp32 operation per step in exactly this order, nothing
// contracted (include/sibrar_hip.h states the same order, tests/ifknn_ref.py derives its bound from it). Both zeros leave as +0.
__device__ __forceinline__ float dknn_value(float dot, float norm_i, float norm_j, float shrinkage) {
#pragma clang fp contract(off)
  const float den = norm_i * norm_j;
  float v = dot / den;
  if (shrinkage > 0.f) {
    const float s = dot / (dot + shrinkage);
    v = v * s;
  }
  const unsigned int b = __float_as_uint(v);
  return (b << 1) == 0u ? 0.f : v;
}

__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ F, long ld, int n, int d, float* __restrict__ norms) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const float* f = F + (long)i * ld;
  float q = 0.f;
  for (int k = 0; k < d; ++k) q = fmaf(f[k], f[k], q);
  norms[i] = sqrtf(q);
}

extern "C" int sbr_row_norms_f32(const float* F, int n, int d, long ld, float* norms, void* stream) {
  SBR_REQUIRE(n >= 0 && d >= 1 && d <= DK_D_MAX && ld >= d, "sbr_row_norms_f32: bad shape (n=%d, d=%d, ld=%ld; 1 <= d <= %d)", n, d, ld, DK_D_MAX);
  if (n == 0) return SBR_OK;
  SBR_REQUIRE(F && norms, "sbr_row_norms_f32: null operand");
  row_norms_kernel<<<(unsigned)sbr_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(F, ld, n, d, norms);
  SBR_CHECK_LAUNCH("sbr_row_norms_f32");
  return SBR_OK;
}

// One wave: the k largest of the n_e (> k) distinct composites of `buf` move to buf[0, k) in no particular order; -> the k-th largest
// (the smallest kept), the same in every lane. Bitwise select from the top bit: T keeps a bit when at least k entries are >= T with it.
__device__ __forceinline__ unsigned long long dknn_reduce(unsigned long long* buf, int n_e, int k, int epl, int lane) {
  unsigned long long e[DK_EPL_MAX];
#pragma unroll
  for (int s = 0; s < DK_EPL_MAX; ++s) {
    const int x = s * 64 + lane;
    e[s] = (s < epl && x < n_e) ? buf[x] : 0ull;
  }
  unsigned long long T = 0ull;
  for (int bit = 63; bit >= 0; --bit) {
    const unsigned long long trial = T | (1ull << bit);
    int c = 0;
#pragma unroll
    for (int s = 0; s < DK_EPL_MAX; ++s) c += __popcll(__ballot(e[s] >= trial));
    if (c >= k) T = trial;
  }
  int base = 0;
#pragma unroll
  for (int s = 0; s < DK_EPL_MAX; ++s) {
    const bool keep = e[s] >= T;                       // (T > 0: it is one of the entries; the empty slots hold 0)
    const unsigned long long m = __ballot(keep);
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < k) buf[pos] = e[s];              // (pos < k always: the guard keeps a wrong count inside the list)
    base += __popcll(m);
  }
  return T;
}

// One workgroup per DK_ROWS query rows i0 ... of [r0, r1). The n candidate rows are covered by column tiles of DK_COLS; per tile
//   product   k-chunks of both operands go through LDS (rows >= n and columns >= d as zeros: what lies there is never multiplied);
//             wave w holds the 32 x 32 dots of the query rows and the tile's candidates 32 w ... in one accumulator;
//   epilogue  every dot != 0 of a row < r1 and a column < n becomes its composite; one above the row's threshold (0 until the first
//             reduction) is appended to the row's buffer of `cap` = kpad + DK_COLS composites;
//   reduce    a row whose buffer could not take another tile is cut to its k largest by the wave that owns it (rows w, w + 4, ...);
//             the k-th becomes the threshold: nothing at or below it can enter the list any more.
// After the last tile the rows are cut to k, sorted (bitonic, descending composites: value descending, index ascending) and written.
__global__ __launch_bounds__(DK_THREADS) void dense_knn_topk_kernel(const float* __restrict__ F, long ld, const float* __restrict__ norms,
                                                                    int n, int d, int r0, int r1, float shrinkage, int k, int kpad,
                                                                    int cap, int* __restrict__ nbr_idx, float* __restrict__ nbr_val,
                                                                    int* __restrict__ nbr_len) {
  extern __shared__ unsigned long long buf[];          // [DK_ROWS][cap]
  __shared__ float As[DK_ROWS][DK_LDP];
  __shared__ float Bs[DK_COLS][DK_LDP];
  __shared__ unsigned long long s_thr[DK_ROWS];
  __shared__ unsigned int s_cnt[DK_ROWS];
  __shared__ float s_ni[DK_ROWS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, l31 = lane & 31, half = lane >> 5;
  const int i0 = r0 + DK_ROWS * (int)blockIdx.x;
  const int epl = cap / 64;
  if (t < DK_ROWS) {
    s_thr[t] = 0ull;
    s_cnt[t] = 0u;
    s_ni[t] = i0 + t < n ? norms[i0 + t] : 0.f;
  }
  // the staging slots of this thread: column kx of the chunk, rows ry, ry + 8, ...
  const int kx = t & 31, ry = t >> 5;
  const int n_chunks = (d + DK_KC - 1) / DK_KC;
  float ra[DK_ROWS / 8], rb[DK_COLS / 8];
  auto fetch = [&](int j0, int c) {
    const int kg = c * DK_KC + kx;
    const bool kin = kg < d;
#pragma unroll
    for (int q = 0; q < DK_ROWS / 8; ++q) {
      const int gi = i0 + ry + 8 * q;
      ra[q] = (kin && gi < n) ? F[(long)gi * ld + kg] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < DK_COLS / 8; ++q) {
      const int gj = j0 + ry + 8 * q;
      rb[q] = (kin && gj < n) ? F[(long)gj * ld + kg] : 0.f;
    }
  };
  __syncthreads();

  for (int j0 = 0; j0 < n; j0 += DK_COLS) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    fetch(j0, 0);
    for (int c = 0; c < n_chunks; ++c) {
      __syncthreads();                                 // the chunk before has been read
#pragma unroll
      for (int q = 0; q < DK_ROWS / 8; ++q) As[ry + 8 * q][kx] = ra[q];
#pragma unroll
      for (int q = 0; q < DK_COLS / 8; ++q) Bs[ry + 8 * q][kx] = rb[q];
      __syncthreads();
      if (c + 1 < n_chunks) fetch(j0, c + 1);          // in flight under the MFMAs
#pragma unroll 4
      for (int kk = 0; kk < DK_KC; kk += 2) {
        const float a = As[l31][kk + half], b = Bs[32 * w + l31][kk + half];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
    }
    // ---- epilogue: accumulator register r is row (r & 3) + 8 (r >> 2) + 4 half, column lane & 31
    const int j = j0 + 32 * w + l31;
    const float nj = j < n ? norms[j] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
      const int i = i0 + row;
      const float dot = acc[r];
      if (i < r1 && j < n && dot != 0.f) {
        const float v = i == j ? 0.f : dknn_value(dot, s_ni[row], nj, shrinkage);
        const unsigned long long e = ((unsigned long long)st_f2key(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)j);
        if (e > s_thr[row]) {
          const unsigned int pos = atomicAdd(&s_cnt[row], 1u);
          if (pos < (unsigned int)cap) buf[(long)row * cap + pos] = e;      // (pos < cap always: see the reduction's condition)
        }
      }
    }
    __syncthreads();
    // ---- reduce the rows that cannot take another tile
    for (int row = w; row < DK_ROWS; row += DK_WAVES) {
      const int n_e = (int)s_cnt[row];
      if (n_e > cap - DK_COLS) {                       // cap - DK_COLS >= k: more than k entries
        const unsigned long long T = dknn_reduce(buf + (long)row * cap, n_e, k, epl, lane);
        if (lane == 0) { s_cnt[row] = (unsigned int)k; s_thr[row] = T; }
      }
    }
    __syncthreads();
  }

  // ---- cut to k, pad, sort, write
  for (int row = w; row < DK_ROWS; row += DK_WAVES) {
    const int n_e = (int)s_cnt[row];
    if (n_e > k) {
      dknn_reduce(buf + (long)row * cap, n_e, k, epl, lane);
      if (lane == 0) s_cnt[row] = (unsigned int)k;
    }
  }
  __syncthreads();
  for (int x = t; x < DK_ROWS * kpad; x += DK_THREADS) {
    const int row = x / kpad, s = x - row * kpad;
    if (s >= (int)s_cnt[row]) buf[(long)row * cap + s] = 0ull;
  }
  __syncthreads();
  for (int size = 2; size <= kpad; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int x = t; x < DK_ROWS * kpad; x += DK_THREADS) {
        const int row = x / kpad, s = x - row * kpad, p = s ^ stride;
        if (p > s) {
          unsigned long long* l = buf + (long)row * cap;
          const bool desc = (s & size) == 0;
          const unsigned long long a = l[s], b = l[p];
          if ((a < b) == desc) { l[s] = b; l[p] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int x = t; x < DK_ROWS * k; x += DK_THREADS) {
    const int row = x / k, s = x - row * k, i = i0 + row;
    if (i >= r1) continue;
    const unsigned long long e = buf[(long)row * cap + s];
    const bool real = s < (int)s_cnt[row];
    nbr_idx[(long)i * k + s] = real ? (int)(0xFFFFFFFFu - (unsigned int)(e & 0xFFFFFFFFull)) : -1;
    nbr_val[(long)i * k + s] = real ? st_key2f((unsigned int)(e >> 32)) : 0.f;
  }
  if (t < DK_ROWS && i0 + t < r1) nbr_len[i0 + t] = (int)s_cnt[t];
}

extern "C" int sbr_dense_knn_topk(const float* F, const float* norms, int n, int d, long ld, int r0, int r1, float shrinkage, int k,
                                  int* nbr_idx, float* nbr_val, int* nbr_len, void* stream) {
  SBR_REQUIRE(k >= 1 && k <= DK_K_MAX, "sbr_dense_knn_topk: k=%d outside [1, %d]", k, DK_K_MAX);
  SBR_REQUIRE(d >= 1 && d <= DK_D_MAX, "sbr_dense_knn_topk: d=%d outside [1, %d]", d, DK_D_MAX);
  SBR_REQUIRE(ld >= d, "sbr_dense_knn_topk: leading dimension %ld below d=%d", ld, d);
  SBR_REQUIRE(shrinkage >= 0.f, "sbr_dense_knn_topk: negative shrinkage %g", (double)shrinkage);
  SBR_REQUIRE(n >= 0 && (long)n * k < (1L << 31), "sbr_dense_knn_topk: n=%d rows of k=%d entries, outside n >= 0, n k < 2^31", n, k);
  SBR_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= n, "sbr_dense_knn_topk: row range [%d, %d) outside [0, %d]", r0, r1, n);
  if (r0 == r1) return SBR_OK;
  SBR_REQUIRE(F && norms && nbr_idx && nbr_val && nbr_len, "sbr_dense_knn_topk: null operand");
  int kpad = 64;                                       // a power of two: the sort's size; a multiple of 64: whole entries per lane
  while (kpad < k) kpad <<= 1;
  const int cap = kpad + DK_COLS;
  const size_t lds = (size_t)DK_ROWS * cap * 8;
  static SbrLdsSlot lds_slot;
  const int rc = sbr_raise_lds("sbr_dense_knn_topk", (const void*)dense_knn_topk_kernel, &lds_slot, lds);
  if (rc) return rc;
  dense_knn_topk_kernel<<<(unsigned)sbr_cdiv(r1 - r0, DK_ROWS), DK_THREADS, lds, (hipStream_t)stream>>>(
      F, ld, norms, n, d, r0, r1, shrinkage, k, kpad, cap, nbr_idx, nbr_val, nbr_len);
  SBR_CHECK_LAUNCH("sbr_dense_knn_topk");
  return SBR_OK;
}
