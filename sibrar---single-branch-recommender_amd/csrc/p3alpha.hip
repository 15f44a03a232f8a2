// P3alpha (algorithms/graph_algs.py:9-88, Cooper et al., WWW 2014): the three-step random walk on 0/1 interaction data. The users x items
// block of the reference's P^3 is (D_u^-1 X)(D_i^-1 X^T)(D_u^-1 X), so the model is the item-item matrix of the last two factors:
//   sbr_p3_walk_dense  W[i, j] = inv(d_i) * sum over the users v of item i, ascending, of inv(d_v) [j in items(v)]     (graph_algs.py:35-59)
//   sbr_p3_score_rows  out[b, j] = (inv(d_u) * sum over the items i of u = rows[b], ascending, of W[i, j]) ^ alpha      (graph_algs.py:59-68)
// No float atomics: every accumulator has one owner (one lane of one wave at a time, the wave's program order between two users; one
// thread in the score rows) and receives its terms in the order stated above by plain fp32 additions, so both give the same bits on
// every run and are valid in deterministic mode. include/sibrar_hip.h states the same order; tests/p3alpha_ref.py restates it in numpy.
#include "common.h"
#include "csr_walk.h"

#define P3_THREADS 1024
#define P3_WAVES (P3_THREADS / 64)
#define P3_DIM_MAX (1 << 24)         // a degree is at most a dimension of X: converted to fp32 exactly

// inv(d) of the header: one correctly rounded fp32 division of an exactly converted degree
__device__ __forceinline__ float p3_inv(long d) { return 1.0f / (float)d; }

// One workgroup per row i of W. (indptr, indices) is X (a user's items), (t_indptr, t_indices) is X^T (row i: the users of item i). A
// tile of tw columns lives in LDS, cut into one strip of `strip` columns per wave. Every wave walks ALL users of item i in ascending
// order by itself: 64 of them at a time are loaded one per lane (1 / d_v, and where the user's item list enters the strip, by a lower
// bound), then taken one after the other with the lanes across the user's items inside the strip. Within one user the columns are
// distinct, so no two lanes meet; between two users the wave's program order (a wave-level fence) fixes the sequence. So a strip needs
// neither atomics nor a workgroup barrier per user, and column j sees inv(d_v) in ascending v whatever the tiling.
__global__ __launch_bounds__(P3_THREADS) void p3_walk_dense_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                                   const long* __restrict__ t_indptr, const int* __restrict__ t_indices,
                                                                   int m, int r0, int tw, int strip, float* __restrict__ W, long ld) {
#pragma clang fp contract(off)
  extern __shared__ float acc_all[];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i = r0 + (int)blockIdx.x;
  const long u_beg = t_indptr[i], u_end = t_indptr[i + 1];
  const float inv_i = p3_inv(u_end - u_beg);
  float* row = W + (long)i * ld;
  for (int t0 = 0; t0 < m; t0 += tw) {
    const int width = t0 + tw < m ? tw : m - t0;
    for (int x = t; x < width; x += P3_THREADS) acc_all[x] = 0.f;
    __syncthreads();
    const int s_beg = w * strip;                                  // this wave's strip: tile columns [s_beg, s_beg + s_width)
    const int s_width = s_beg >= width ? 0 : (s_beg + strip < width ? strip : width - s_beg);
    if (s_width > 0) {
      const int c0 = t0 + s_beg;                                  // first column of the strip
      float* acc = acc_all + s_beg;
      for (long p0 = u_beg; p0 < u_end; p0 += 64) {
        const int n_e = u_end - p0 < 64 ? (int)(u_end - p0) : 64;
        long my_lo = 0, my_end = 0;
        float my_inv = 0.f;
        if (lane < n_e) {
          const int v = t_indices[p0 + lane];
          my_lo = indptr[v];
          my_end = indptr[v + 1];
          my_inv = p3_inv(my_end - my_lo);
          if (c0 > 0) my_lo = sbr_csr_lower_bound(indices, my_lo, my_end, c0);
        }
        for (int e = 0; e < n_e; ++e) {
          const float iv = __shfl(my_inv, e, 64);
          const long end = __shfl(my_end, e, 64);
          sbr_csr_walk_window(indices, __shfl(my_lo, e, 64), end, c0, s_width, lane, [&](unsigned int x, long) { acc[x] = acc[x] + iv; });
          // the next user may name the same accumulator from another lane: keep the LDS accesses of two users in program order
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    __syncthreads();
    for (int x = t; x < width; x += P3_THREADS) row[t0 + x] = u_end > u_beg ? acc_all[x] * inv_i : 0.f;
    __syncthreads();
  }
}

extern "C" int sbr_p3_walk_dense(const long* indptr, const int* indices, const long* t_indptr, const int* t_indices, int n, int m, int r0,
                                 int r1, int tile_cols, float* W, long ld, void* stream) {
  SBR_REQUIRE(n >= 0 && n <= P3_DIM_MAX && m >= 0 && m <= P3_DIM_MAX, "sbr_p3_walk_dense: shape [%d, %d] outside [0, 2^24] x [0, 2^24]: a "
              "degree over 2^24 has no exact fp32 form", n, m);
  SBR_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= m, "sbr_p3_walk_dense: row range [%d, %d) outside [0, %d]", r0, r1, m);
  SBR_REQUIRE(ld >= m, "sbr_p3_walk_dense: leading dimension %ld below m=%d", ld, m);
  static SbrLdsSlot lds_slot;
  const int tw = sbr_row_tile("sbr_p3_walk_dense", (const void*)p3_walk_dense_kernel, &lds_slot, m, tile_cols, 0, r1 - r0,
                              indptr && indices && t_indptr && t_indices && W);
  if (tw <= 0) return -tw;
  const int strip = (tw + P3_WAVES - 1) / P3_WAVES;
  p3_walk_dense_kernel<<<(unsigned)(r1 - r0), P3_THREADS, 4 * (size_t)tw, (hipStream_t)stream>>>(indptr, indices, t_indptr, t_indices, m, r0, tw,
                                                                                           strip, W, ld);
  SBR_CHECK_LAUNCH("sbr_p3_walk_dense");
  return SBR_OK;
}

// ---- score rows ----------------------------------------------------------------------------------------------------------------------
#define P3S_THREADS 256
#define P3S_COLS 4                   // columns per thread, P3S_THREADS apart: a workgroup owns (user, 1,024 columns)
#define P3S_UNROLL 4                 // rows of W in flight per column

// A thread owns its columns: reads of a row of W are coalesced across the workgroup, and a column's accumulator receives W[i, j] over
// the user's items i in ascending order (the loads of P3S_UNROLL rows are issued together, the additions stay in order).
__global__ __launch_bounds__(P3S_THREADS) void p3_score_rows_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                                    const long* __restrict__ rows, const float* __restrict__ W, long ldw,
                                                                    int m, int col_blocks, float alpha, float* __restrict__ out, long ldo) {
#pragma clang fp contract(off)
  const long b = (long)blockIdx.x / col_blocks;
  const int j0 = (int)((long)blockIdx.x % col_blocks) * (P3S_THREADS * P3S_COLS) + (int)threadIdx.x;
  const long u = rows ? rows[b] : b;
  const long p_beg = indptr[u], p_end = indptr[u + 1];
  float acc[P3S_COLS];
#pragma unroll
  for (int c = 0; c < P3S_COLS; ++c) acc[c] = 0.f;
  long p = p_beg;
  for (; p + P3S_UNROLL <= p_end; p += P3S_UNROLL) {
    float v[P3S_UNROLL][P3S_COLS];
#pragma unroll
    for (int s = 0; s < P3S_UNROLL; ++s) {
      const float* wr = W + (long)indices[p + s] * ldw;
#pragma unroll
      for (int c = 0; c < P3S_COLS; ++c) {
        const int j = j0 + c * P3S_THREADS;
        v[s][c] = j < m ? wr[j] : 0.f;
      }
    }
#pragma unroll
    for (int s = 0; s < P3S_UNROLL; ++s)
#pragma unroll
      for (int c = 0; c < P3S_COLS; ++c) acc[c] = acc[c] + v[s][c];
  }
  for (; p < p_end; ++p) {
    const float* wr = W + (long)indices[p] * ldw;
#pragma unroll
    for (int c = 0; c < P3S_COLS; ++c) {
      const int j = j0 + c * P3S_THREADS;
      if (j < m) acc[c] = acc[c] + wr[j];
    }
  }
  const float inv_u = p3_inv(p_end - p_beg);
  float* o = out + b * ldo;
#pragma unroll
  for (int c = 0; c < P3S_COLS; ++c) {
    const int j = j0 + c * P3S_THREADS;
    if (j >= m) continue;
    float s = p_end > p_beg ? acc[c] * inv_u : 0.f;
    if (alpha != 1.0f) s = s == 0.f ? 0.f : powf(s, alpha);
    o[j] = s;
  }
}

extern "C" int sbr_p3_score_rows(const long* indptr, const int* indices, const long* rows, long B, const float* W, long ldw, int m,
                                 float alpha, float* out, long ldo, void* stream) {
  SBR_REQUIRE(B >= 0 && m >= 0 && m <= P3_DIM_MAX && ldw >= m && ldo >= m, "sbr_p3_score_rows: bad shape (B=%ld, m=%d, ldw=%ld, ldo=%ld)", B,
              m, ldw, ldo);
  SBR_REQUIRE(sbr_pos_finite(alpha), "sbr_p3_score_rows: alpha=%g is not a positive finite power", (double)alpha);
  if (B == 0 || m == 0) return SBR_OK;
  SBR_REQUIRE(indptr && indices && W && out, "sbr_p3_score_rows: null operand");
  const int col_blocks = sbr_cdiv(m, P3S_THREADS * P3S_COLS);
  SBR_REQUIRE(B * col_blocks <= 2147483647L, "sbr_p3_score_rows: B=%ld rows of %d column blocks exceed one grid", B, col_blocks);
  p3_score_rows_kernel<<<(unsigned)(B * col_blocks), P3S_THREADS, 0, (hipStream_t)stream>>>(indptr, indices, rows, W, ldw, m, col_blocks, alpha,
                                                                                   out, ldo);
  SBR_CHECK_LAUNCH("sbr_p3_score_rows");
  return SBR_OK;
}
