// SLIM (algorithms/linear_algs.py:15-127, Ning and Karypis, ICDM 2011): one non-negative elastic net per item column, solved from the
// Gram matrix G = X^T X alone. For the target item j, with q = G[:, j], q_j = 0, and the penalties l1 = n alpha l1_ratio,
// l2 = n alpha (1 - l1_ratio) (n users), sklearn's objective times n is
//   1/2 (G_jj - 2 w.q + w.G w) + l1 sum(w) + 1/2 l2 w.w,   w >= 0, w_j = 0,
// and with the residual r = q - G w the coordinate step for k != j, G_kk > 0 is
//   new = max(r_k + G_kk w_k - l1, 0) / (G_kk + l2);   r <- r - (new - w_k) G[k, :];   w_k <- new.
// sbr_slim_cd_f32 runs cyclic coordinate descent in ascending k, one workgroup per target column, r in LDS, w in the output column.
// No atomics and no float reduction: every element of r and of the column has one owner thread and receives its updates in the order
// of the steps, so the result is the same bits on every run and for every split of the column range, and is valid in deterministic
// mode. include/sibrar_hip.h states the contract; tests/slim_ref.py restates the loop in numpy.
#include "common.h"

#define SLIM_THREADS 1024
#define SLIM_WAVES (SLIM_THREADS / 64)
#define SLIM_NONE 0x7fffffff
#define SLIM_FIRST 4                 // elements of the row G[k, :] per thread whose loads are issued before the step is known
#define SLIM_FIXED 512               // static LDS (the waves' candidates in two buffers, the sweep's verdict: 260 bytes), rounded up
#define SLIM_MAX_M ((SBR_LDS_MAX - SLIM_FIXED) / 4)      // 40,832 items: r [m] beside the static part in 160 KiB

// One workgroup per target column j = c0 + blockIdx.x. Coordinate x belongs to thread x % SLIM_THREADS: that thread alone reads and
// writes r[x] (dynamic LDS) and writes W[x, j], and it keeps "w_x > 0" as bit x / SLIM_THREADS of a register (m <= SLIM_MAX_M: 40 bits).
//
// A sweep walks the coordinates in chunks of SLIM_THREADS. In a turn every thread tests its own coordinate of the chunk, if it lies
// behind the last step taken: can its step be non-zero, i.e. w_x > 0, or r_x > l1 (then G_xx > 0, since an item nobody holds has a zero
// row and column in G and so r_x = 0)? The first such thread of every wave puts its index, its bit and r_x into LDS, and after one
// barrier every thread reads the same first candidate k of the workgroup, or that there is none, which ends the chunk. Every thread
// then computes the step itself from r_k (LDS), G_kk and w_k (uniform loads) and updates its own elements of r; the search goes on
// behind k. A coordinate that is passed over has w_x = 0 and r_x <= l1, i.e. new = 0 = w_x: the plain ascending loop would not have
// changed anything there either.
//
// G is only read here, so the compiler may fetch G_kk (an address that is the same in every lane) through the scalar cache. w_k must
// never take that way: W is written in this kernel, by vector stores, and the scalar cache is not kept coherent with them, so a load
// of w_k through it could return the value of an earlier sweep. W is therefore neither const nor read through a const alias, which
// keeps the load of w_k a vector load; keep it so.
//
// The owner of k stores the new w_k only after the NEXT barrier it passes: every other thread's load of the old w_k lies before that
// barrier, and the next load of w_k, a sweep later, behind a further one. The candidates are double-buffered, so one barrier per turn
// is all there is. Every barrier sits in uniform control flow: what decides it (the candidate, the sweep's verdict) is read from LDS.
__global__ __launch_bounds__(SLIM_THREADS) void slim_cd_kernel(const float* __restrict__ G, int m, long ldg, int c0, float l1, float l2,
                                                               int max_iter, float tol, float* __restrict__ W, long ldw,
                                                               int* __restrict__ n_iter) {
#pragma clang fp contract(off)
  extern __shared__ float r[];
  __shared__ int s_first[2][SLIM_WAVES];
  __shared__ float s_r[2][SLIM_WAVES];
  __shared__ int s_verdict;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int j = c0 + (int)blockIdx.x;
  float* wcol = W + j;

  const float* q = G + (long)j * ldg;                             // G is symmetric: column j is row j
  for (int x = t; x < m; x += SLIM_THREADS) r[x] = x == j ? 0.f : q[x];

  unsigned long long positive = 0ull;                             // bit c: w of coordinate c * SLIM_THREADS + t is > 0
  int pend_k = -1;                                                // the owner's store of w_k that waits for the next barrier
  float pend_w = 0.f;
  int sweeps = 0, par = 0, verdict = 0;
  while (sweeps < max_iter) {                                     // at most max_iter sweeps
    ++sweeps;
    float d_w_max = 0.f, w_max = 0.f;                             // the same in every thread: every thread computes every step
    for (int b = 0, c = 0; b < m; b += SLIM_THREADS, ++c) {
      int lo = 0;                                                 // threads below lo have had their turn in this chunk
      for (int turn = 0; turn <= SLIM_THREADS; ++turn) {          // every turn but a chunk's last raises lo: at most SLIM_THREADS + 1
        const int x = b + t;
        const int had_x = (int)((positive >> c) & 1ull);
        float rx = 0.f;
        bool cand = false;
        if (x < m && t >= lo && x != j) {
          rx = r[x];
          cand = had_x || rx > l1;
        }
        const unsigned long long vote = __ballot(cand);
        const int first_lane = vote ? __ffsll((long long)vote) - 1 : 0;
        if (lane == first_lane) {
          s_first[par][wv] = vote ? (t << 1 | had_x) : SLIM_NONE;
          s_r[par][wv] = rx;
        }
        __syncthreads();
        if (pend_k >= 0) {
          wcol[(long)pend_k * ldw] = pend_w;
          pend_k = -1;
        }
        int found = SLIM_NONE;
#pragma unroll
        for (int w2 = SLIM_WAVES - 1; w2 >= 0; --w2) {
          const int f = s_first[par][w2];
          found = f != SLIM_NONE ? f : found;                     // the lowest wave that has one
        }
        if (found == SLIM_NONE) {
          par ^= 1;
          break;
        }
        const int first = found >> 1;
        const int k = b + first;
        const float rk = s_r[par][first >> 6];
        par ^= 1;                                                 // the next turn writes the other buffer: no barrier behind these reads
        const float* row = G + (long)k * ldg;
        float g[SLIM_FIRST];
#pragma unroll
        for (int u = 0; u < SLIM_FIRST; ++u) {
          const int y = t + u * SLIM_THREADS;
          g[u] = y < m ? row[y] : 0.f;
        }
        const float gkk = row[k];
        const float wk = (found & 1) ? wcol[(long)k * ldw] : 0.f;
        float nw = wk;
        if (gkk > 0.f) {                                          // a zero-norm column is skipped, as in sklearn
          const float num = (rk + gkk * wk) - l1;
          nw = (num > 0.f ? num : 0.f) / (gkk + l2);
        }
        const float d = nw - wk;
        if (d != 0.f) {
#pragma unroll
          for (int u = 0; u < SLIM_FIRST; ++u) {
            const int y = t + u * SLIM_THREADS;
            if (y < m) r[y] = r[y] - d * g[u];
          }
          for (int y = t + SLIM_FIRST * SLIM_THREADS; y < m; y += SLIM_THREADS) r[y] = r[y] - d * row[y];
          if (t == first) {                                       // the owner of k
            pend_k = k;
            pend_w = nw;
            positive = nw > 0.f ? (positive | (1ull << c)) : (positive & ~(1ull << c));
          }
        }
        d_w_max = fmaxf(d_w_max, fabsf(d));
        w_max = fmaxf(w_max, fabsf(nw));
        lo = first + 1;
      }
    }
    // sklearn's first stopping test (its dual-gap test is not reproduced): thread 0 decides, LDS tells
    if (t == 0) s_verdict = (w_max == 0.f || d_w_max <= tol * w_max) ? 1 : 0;
    __syncthreads();
    if (pend_k >= 0) {
      wcol[(long)pend_k * ldw] = pend_w;
      pend_k = -1;
    }
    verdict = s_verdict;
    __syncthreads();                                              // the next sweep loads w behind the stores above, and s_verdict is free
    if (verdict) break;
  }
  // every element of the column is written: a coordinate without the bit is zero (its owner stored at most a zero there before)
  for (int x = t, c = 0; x < m; x += SLIM_THREADS, ++c)
    if (!((positive >> c) & 1ull)) wcol[(long)x * ldw] = 0.f;
  if (t == 0) n_iter[j] = verdict ? sweeps : -sweeps;
}

extern "C" int sbr_slim_cd_f32(const float* G, int m, long ldg, int c0, int c1, float l1, float l2, int max_iter, float tol, float* W,
                               long ldw, int* n_iter, void* stream) {
  SBR_REQUIRE(m >= 0 && m <= SLIM_MAX_M, "sbr_slim_cd_f32: m=%d outside [0, %d]: the residual of a column, 4 m bytes, lives in the 160 KiB "
              "of LDS", m, SLIM_MAX_M);
  SBR_REQUIRE(c0 >= 0 && c0 <= c1 && c1 <= m, "sbr_slim_cd_f32: column range [%d, %d) outside [0, %d]", c0, c1, m);
  SBR_REQUIRE(ldg >= m && ldw >= m, "sbr_slim_cd_f32: leading dimensions %ld, %ld below m=%d", ldg, ldw, m);
  SBR_REQUIRE(l1 >= 0.f && l1 <= 3.402823466e+38f && l2 >= 0.f && l2 <= 3.402823466e+38f,
              "sbr_slim_cd_f32: the penalties l1=%g, l2=%g must be finite and not negative", (double)l1, (double)l2);
  SBR_REQUIRE(tol >= 0.f && tol <= 3.402823466e+38f, "sbr_slim_cd_f32: tol=%g must be finite and not negative", (double)tol);
  SBR_REQUIRE(max_iter >= 1, "sbr_slim_cd_f32: max_iter=%d below 1", max_iter);
  static SbrLdsSlot lds_slot;
  const int tw = sbr_row_tile("sbr_slim_cd_f32", (const void*)slim_cd_kernel, &lds_slot, m, m, SLIM_FIXED, c1 - c0, G && W && n_iter);
  if (tw <= 0) return -tw;
  slim_cd_kernel<<<(unsigned)(c1 - c0), SLIM_THREADS, 4 * (size_t)m, (hipStream_t)stream>>>(G, m, ldg, c0, l1, l2, max_iter, tol, W, ldw,
                                                                                         n_iter);
  SBR_CHECK_LAUNCH("sbr_slim_cd_f32");
  return SBR_OK;
}
