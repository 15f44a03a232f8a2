// Truncated SVD by block subspace iteration (algorithms/mf_algs.py:14-66, where the reference calls ARPACK through scipy's svds). One
// half-iteration is a sparse product, the Gram matrix of its result, that matrix's eigen-decomposition and a rotation:
//   sbr_csr_times_dense_f32  Y = X V (or Z = X^T U): a CSR matrix times a dense block of at most 128 columns
//   sbr_gram_f32             G = Y^T Y                (csrc/als.hip: the slab kernel of sbr_als_gram_f32, nothing added to the diagonal)
//   sbr_sym_eig_f32          G = W diag(lam) W^T      parallel cyclic Jacobi by one workgroup, in double, lam descending
//   sbr_rotate_cols_f32      Y W diag(1 / s), s = sqrt(max(lam, tiny)): the orthonormal basis (also U <- U W, without the scale)
//   sbr_col_residual_f32     ||Y[:, j] - s_j U[:, j]||_2 per column: the stopping rule
// No float atomics anywhere: every output element has one owner and receives its terms in a stated order (include/sibrar_hip.h), so
// every entry gives the same bits on every run and is valid in deterministic mode. csr_walk.h is not used: its walkers enter a sorted
// row inside a window of columns, and these products take whole rows. tests/svd_ref.py restates the iteration in float32 numpy.
#include "block128.h"

// ---- out[r, 0:c] = sum_k data_k D[col_k, 0:c] ---------------------------------------------------------------------------------------
#define CTD_THREADS 256               // four waves, a wave owns a row (block128.h: SbrRow2)

__global__ __launch_bounds__(CTD_THREADS) void csr_times_dense_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                                      const float* __restrict__ data, long r0, long r1,
                                                                      const float* __restrict__ D, long ldd, int c, float* __restrict__ out,
                                                                      long ldo) {
#pragma clang fp contract(off)
  const SbrRow2 w(c);
  const long r = r0 + (long)blockIdx.x * (CTD_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= r1) return;
  const long beg = indptr[r], end = indptr[r + 1];
  float a0 = 0.f, a1 = 0.f;
  long p = beg;
  for (; p + 4 <= end; p += 4) {                                    // four rows of D in flight; the terms still enter in CSR order
    float v[4], x0[4], x1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* d = D + (long)indices[p + u] * ldd;
      v[u] = data ? data[p + u] : 1.f;
      w.load(d, x0[u], x1[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a0 = fmaf(v[u], x0[u], a0);
      a1 = fmaf(v[u], x1[u], a1);
    }
  }
  for (; p < end; ++p) {
    const float* d = D + (long)indices[p] * ldd;
    const float v = data ? data[p] : 1.f;
    float x0, x1;
    w.load(d, x0, x1);
    a0 = fmaf(v, x0, a0);
    a1 = fmaf(v, x1, a1);
  }
  w.store(out + r * ldo, a0, a1);
}

extern "C" int sbr_csr_times_dense_f32(const long* indptr, const int* indices, const float* data, long r0, long r1, const float* D, long n_d,
                                       long ldd, int c, float* out, long ldo, void* stream) {
  SBR_REQUIRE_WIDTH(__func__, "c", c);
  SBR_TRY(sbr_check_ld(__func__, "c", c, {{"ldd", ldd}, {"ldo", ldo}}));
  SBR_REQUIRE_ROWS(__func__, r0, r1, 2147483646L);
  SBR_REQUIRE(n_d >= 0, "%s: n_d=%ld is negative", __func__, n_d);
  if (r0 == r1) return SBR_OK;
  SBR_REQUIRE_OPERANDS(__func__, indptr && out && (n_d == 0 || D));                                  // (a matrix without entries has no indices)
  csr_times_dense_kernel<<<(unsigned)sbr_slabs(r1 - r0, CTD_THREADS / 64), CTD_THREADS, 0, (hipStream_t)stream>>>(indptr, indices, data, r0, r1, D, ldd,
                                                                                                          c, out, ldo);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}

// ---- A = W diag(lam) W^T by parallel cyclic Jacobi, one workgroup -------------------------------------------------------------------
// The matrix is fp32, the iteration is in double and the results are rounded once: a float32 Jacobi iteration applies about a thousand
// rotations to every column at n = 128 and leaves errors of 1e-6, forty times what the rounding of the results costs.
#define EIG_THREADS 512
#define EIG_MAX_SWEEPS 30             // the sweep cap of include/sibrar_hip.h
#define EIG_EPS 0x1p-40               // a pair is left alone when |a_pq| <= EIG_EPS * sqrt(|a_pp| |a_qq|)
#define EIG_PAIRS (SBR_BLOCK_MAX / 2)

// n is padded to the even np = n + (n & 1): the extra index of an odd n is the bye, a zero row and column that no rotation touches.
// Odd row stride: the elements of a column, and the scattered elements of a step's 2 x 2 blocks, spread over the banks.
__host__ __device__ static inline int eig_np(int n) { return (n + 1) & ~1; }
__host__ __device__ static inline int eig_ld(int n) { return sbr_odd_ld(eig_np(n)); }
static inline size_t eig_lds_bytes(int n) { return 8 * (sbr_odd_cells(eig_np(n), eig_np(n)) + 4 * EIG_PAIRS + SBR_BLOCK_MAX) + 4 * (3 * EIG_PAIRS + SBR_BLOCK_MAX + 4); }

extern "C" long sbr_sym_eig_f32_workspace(int n) {
  if (n < 1 || n > SBR_BLOCK_MAX) return 0;
  return 8L * eig_np(n) * eig_np(n);
}

// LDS (double): A [np][ld] the matrix, symmetric bit for bit throughout | cs, sn [64] the step's rotations | dp, dq [64] the rotated
// pairs' new diagonal elements | sg [128] a column's sign over its length; (int): pi, qi [64] the step's pairs | on [64] 1: the pair is
// rotated in this step | perm [128] the column of W that becomes output column c | flag [1] a rotation happened in this sweep.
// Global (double): Wt [np][np], the accumulated rotations, transposed (a column of W is contiguous): A and W in double do not both fit
// the 160 KiB, and W is only ever walked along its columns. One workgroup: what it stores is visible to it behind a barrier.
__global__ __launch_bounds__(EIG_THREADS) void sym_eig_kernel(const float* __restrict__ Ain, long lda, int n, float* __restrict__ Wout, long ldw,
                                                              float* __restrict__ lam, int* __restrict__ info, double* Wt) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) double eig_lds[];
  const int np = eig_np(n), m = np >> 1, ld = eig_ld(n), t = threadIdx.x;
  double* A = eig_lds;
  double* cs = A + np * ld;
  double* sn = cs + EIG_PAIRS;
  double* dp = sn + EIG_PAIRS;
  double* dq = dp + EIG_PAIRS;
  double* sg = dq + EIG_PAIRS;
  int* pi = (int*)(sg + SBR_BLOCK_MAX);
  int* qi = pi + EIG_PAIRS;
  int* on = qi + EIG_PAIRS;
  int* perm = on + EIG_PAIRS;
  int* flag = perm + SBR_BLOCK_MAX;
  // the lower triangle of the n x n view is read, and mirrored
  for (int e = t; e < np * np; e += EIG_THREADS) {
    const int i = e / np, j = e - i * np;
    A[i * ld + j] = (i < n && j < n) ? (double)Ain[(long)(i > j ? i : j) * lda + (i > j ? j : i)] : 0.0;
    Wt[e] = i == j ? 1.0 : 0.0;
  }
  if (t < SBR_BLOCK_MAX) perm[t] = 0;
  if (t == 0) flag[0] = 0;
  __syncthreads();
  bool converged = false;
  for (int sweep = 0; sweep < EIG_MAX_SWEEPS && !converged; ++sweep) {
    for (int r = 0; r < np - 1; ++r) {
      // ---- the pairs of step r (round robin: index np - 1 stays, the others move round) and their rotations ----
      if (t < m) {
        const int a = t == 0 ? r : (r + t) % (np - 1), b = t == 0 ? np - 1 : (r - t + np - 1) % (np - 1);
        const int p = a < b ? a : b, q = a < b ? b : a;
        const double app = A[p * ld + p], aqq = A[q * ld + q], apq = A[p * ld + q];
        double c = 1.0, s = 0.0, np_ = app, nq_ = aqq;
        int rotate = 0;
        if (fabs(apq) > EIG_EPS * (sqrt(fabs(app)) * sqrt(fabs(aqq)))) {
          const double tau = (aqq - app) / (2.0 * apq);
          const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + tt * tt);
          s = tt * c;
          np_ = app - tt * apq;
          nq_ = aqq + tt * apq;
          rotate = 1;
          flag[0] = 1;
        }
        pi[t] = p; qi[t] = q; cs[t] = c; sn[t] = s; dp[t] = np_; dq[t] = nq_; on[t] = rotate;
      }
      __syncthreads();
      // ---- A <- J^T A J, one owner per 2 x 2 block (pair k's rows, pair k2's columns) and its mirror image; the unordered pairs
      // {k, k2} are enumerated as k2 = k + d mod m, d = 0 .. m / 2 ----
      for (int e = t; e < (m / 2 + 1) * m; e += EIG_THREADS) {
        const int d = e / m, k = e - d * m;
        if (2 * d == m && k >= d) continue;                         // an even m meets every block of d = m / 2 twice
        const int k2 = k + d >= m ? k + d - m : k + d;
        if (!on[k] && !on[k2]) continue;
        const int p = pi[k], q = qi[k];
        if (d == 0) {
          A[p * ld + p] = dp[k];
          A[q * ld + q] = dq[k];
          A[p * ld + q] = 0.0;
          A[q * ld + p] = 0.0;
          continue;
        }
        const int p2 = pi[k2], q2 = qi[k2];
        const double c = cs[k], s = sn[k], c2 = cs[k2], s2 = sn[k2];
        const double b00 = A[p * ld + p2], b01 = A[p * ld + q2], b10 = A[q * ld + p2], b11 = A[q * ld + q2];
        const double r00 = c * b00 - s * b10, r10 = s * b00 + c * b10, r01 = c * b01 - s * b11, r11 = s * b01 + c * b11;
        const double n00 = c2 * r00 - s2 * r01, n01 = s2 * r00 + c2 * r01, n10 = c2 * r10 - s2 * r11, n11 = s2 * r10 + c2 * r11;
        A[p * ld + p2] = n00; A[p2 * ld + p] = n00;
        A[p * ld + q2] = n01; A[q2 * ld + p] = n01;
        A[q * ld + p2] = n10; A[p2 * ld + q] = n10;
        A[q * ld + q2] = n11; A[q2 * ld + q] = n11;
      }
      // ---- W <- W J: the lanes of a wave walk down one pair of columns ----
      for (int e = t; e < m * n; e += EIG_THREADS) {
        const int k = e / n, i = e - k * n;
        if (!on[k]) continue;
        const int p = pi[k], q = qi[k];
        const double c = cs[k], s = sn[k], w0 = Wt[p * np + i], w1 = Wt[q * np + i];
        Wt[p * np + i] = c * w0 - s * w1;
        Wt[q * np + i] = s * w0 + c * w1;
      }
      __syncthreads();
    }
    converged = flag[0] == 0;
    __syncthreads();
    if (t == 0) flag[0] = 0;
    __syncthreads();
  }
  // ---- descending order (ties: the lower index first), unit length, the sign rule on the rounded components, the results ----
  if (t < n) {
    const double mine = A[t * ld + t];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double other = A[j * ld + j];
      rank += (other > mine || (other == mine && j < t)) ? 1 : 0;
    }
    perm[rank] = t;
    double len = 0.0;
    for (int i = 0; i < n; ++i) len = fma(Wt[t * np + i], Wt[t * np + i], len);
    const double scale = 1.0 / sqrt(len);
    float best = -1.f, at = 1.f;
    for (int i = 0; i < n; ++i) {
      const float w = (float)(Wt[t * np + i] * scale);
      if (fabsf(w) > best) { best = fabsf(w); at = w; }
    }
    sg[t] = at < 0.f ? -scale : scale;
  }
  __syncthreads();
  for (int e = t; e < n * n; e += EIG_THREADS) {
    const int i = e / n, c = e - i * n, src = perm[c];
    Wout[(long)i * ldw + c] = (float)(Wt[src * np + i] * sg[src]);
  }
  if (t < n) lam[t] = (float)A[perm[t] * ld + perm[t]];
  if (t == 0 && !converged) sbr_report_first(info, EIG_MAX_SWEEPS + 1);
}

extern "C" int sbr_sym_eig_f32(const float* A, int n, long lda, float* W, long ldw, float* lam, int* info, void* workspace, long workspace_bytes,
                               void* stream) {
  SBR_REQUIRE_WIDTH(__func__, "n", n);
  SBR_TRY(sbr_check_ld(__func__, "n", n, {{"lda", lda}, {"ldw", ldw}}));
  SBR_REQUIRE_OPERANDS(__func__, A && W && lam && info);
  SBR_REQUIRE_WORKSPACE(__func__, workspace, workspace_bytes, sbr_sym_eig_f32_workspace(n), 8);
  SBR_RAISE_LDS(sym_eig_kernel, eig_lds_bytes(SBR_BLOCK_MAX));
  sym_eig_kernel<<<1, EIG_THREADS, eig_lds_bytes(n), (hipStream_t)stream>>>(A, lda, n, W, ldw, lam, info, (double*)workspace);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}

// ---- out = Y W diag(1 / s) ----------------------------------------------------------------------------------------------------------
#define ROT_THREADS 256               // 8 x 32 tiles of 4 rows x 4 columns (columns tc, tc + 32, tc + 64, tc + 96)
#define ROT_ROWS 32                   // rows of Y per workgroup
#define ROT_WS 128                    // floats per staged row of W: a wave reads 32 consecutive ones, no bank twice
#define ROT_YS 132                    // floats per staged row of Y: the two rows a wave reads at once lie 4 * 132 floats apart, 16 banks
#define ROT_TINY_REL 1.4210855e-14f   // 2^-46: s_j = sqrt(max(lam_j, max(lam_0 * 2^-46, FLT_MIN)))
static inline size_t rot_lds_bytes(int b) { return 4 * ((size_t)b * ROT_WS + ROT_ROWS * ROT_YS + SBR_BLOCK_MAX); }

// Y and out may be the same matrix: a workgroup stages its rows before it writes them
__global__ __launch_bounds__(ROT_THREADS) void rotate_cols_kernel(const float* Y, long n, long ldy, int b, const float* __restrict__ W, long ldw,
                                                                  const float* __restrict__ lam, float* __restrict__ s_out, float* out,
                                                                  long ldo) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float rot_lds[];
  float* ws = rot_lds;
  float* ys = ws + b * ROT_WS;
  float* inv = ys + ROT_ROWS * ROT_YS;
  const int t = threadIdx.x, tr = t >> 5, tc = t & 31;
  const long row0 = (long)blockIdx.x * ROT_ROWS;
  const int nr = n - row0 < ROT_ROWS ? (int)(n - row0) : ROT_ROWS;
  for (int e = t; e < b * ROT_WS; e += ROT_THREADS) {
    const int k = e / ROT_WS, j = e - k * ROT_WS;
    ws[e] = j < b ? W[(long)k * ldw + j] : 0.f;
  }
  for (int e = t; e < ROT_ROWS * b; e += ROT_THREADS) {
    const int rr = e / b, k = e - rr * b;
    ys[rr * ROT_YS + k] = rr < nr ? Y[(row0 + rr) * ldy + k] : 0.f;
  }
  if (t < SBR_BLOCK_MAX) {
    float iv = 1.f;
    if (lam && t < b) {
      const float s = sqrtf(fmaxf(lam[t], fmaxf(lam[0] * ROT_TINY_REL, 1.17549435e-38f)));
      iv = 1.f / s;
      if (blockIdx.x == 0) s_out[t] = s;
    }
    inv[t] = iv;
  }
  __syncthreads();
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
  for (int k = 0; k < b; ++k) {
    float y[4], w[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) y[a] = ys[(tr * 4 + a) * ROT_YS + k];
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = ws[k * ROT_WS + tc + 32 * c];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = fmaf(y[a], w[c], acc[a][c]);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int rr = tr * 4 + a, j = tc + 32 * c;
      if (rr < nr && j < b) out[(row0 + rr) * ldo + j] = acc[a][c] * inv[j];
    }
}

extern "C" int sbr_rotate_cols_f32(const float* Y, long n, long ldy, int b, const float* W, long ldw, const float* lam, float* s, float* out,
                                   long ldo, void* stream) {
  SBR_REQUIRE_WIDTH(__func__, "b", b);
  SBR_REQUIRE_SLAB_ROWS(__func__, "n", n, ROT_ROWS);
  SBR_TRY(sbr_check_ld(__func__, "b", b, {{"ldy", ldy}, {"ldw", ldw}, {"ldo", ldo}}));
  SBR_REQUIRE_OPERANDS(__func__, W && (!lam || s) && (n == 0 || (Y && out)));
  SBR_RAISE_LDS(rotate_cols_kernel, rot_lds_bytes(SBR_BLOCK_MAX));
  const long tiles = sbr_slabs(n, ROT_ROWS);                        // a workgroup without rows still writes s
  rotate_cols_kernel<<<(unsigned)(tiles > 0 ? tiles : 1), ROT_THREADS, rot_lds_bytes(b), (hipStream_t)stream>>>(Y, n, ldy, b, W, ldw, lam, s, out,
                                                                                                           ldo);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}

// ---- res[j] = ||Y[:, j] - s_j U[:, j]||_2 -------------------------------------------------------------------------------------------
#define RES_SLAB 256                  // rows per workgroup: one partial sum of squares per column and slab, added in slab order

__global__ __launch_bounds__(SBR_BLOCK_MAX) void col_residual_slab_kernel(const float* __restrict__ Y, long ldy, const float* __restrict__ U, long ldu,
                                                                      const float* __restrict__ s, long n, int f, float* __restrict__ ws) {
#pragma clang fp contract(off)
  const int j = threadIdx.x;
  if (j >= f) return;
  const long lo = (long)blockIdx.x * RES_SLAB, hi = lo + RES_SLAB < n ? lo + RES_SLAB : n;
  const float sj = s[j];
  float acc = 0.f;
#pragma unroll 8
  for (long r = lo; r < hi; ++r) {
    const float d = fmaf(-sj, U[r * ldu + j], Y[r * ldy + j]);
    acc = fmaf(d, d, acc);
  }
  ws[(long)blockIdx.x * f + j] = acc;
}

extern "C" long sbr_col_residual_f32_workspace(long n, int f) {
  if (n <= 0 || f < 1 || f > SBR_BLOCK_MAX) return 0;
  return sbr_slab_ws_bytes(n, RES_SLAB, f);
}

extern "C" int sbr_col_residual_f32(const float* Y, long ldy, const float* U, long ldu, const float* s, long n, int f, float* res, void* workspace,
                                    long workspace_bytes, void* stream) {
  SBR_REQUIRE_WIDTH(__func__, "f", f);
  SBR_REQUIRE_SLAB_ROWS(__func__, "n", n, RES_SLAB);
  SBR_TRY(sbr_check_ld(__func__, "f", f, {{"ldy", ldy}, {"ldu", ldu}}));
  SBR_REQUIRE_OPERANDS(__func__, res && s && (n == 0 || (Y && U)));
  SBR_REQUIRE_WORKSPACE(__func__, workspace, workspace_bytes, sbr_col_residual_f32_workspace(n, f), 4);
  const int n_slabs = (int)sbr_slabs(n, RES_SLAB);
  if (n_slabs > 0) {
    col_residual_slab_kernel<<<(unsigned)n_slabs, SBR_BLOCK_MAX, 0, (hipStream_t)stream>>>(Y, ldy, U, ldu, s, n, f, (float*)workspace);
    SBR_CHECK_LAUNCH(__func__);
  }
  sbr_slab_reduce_kernel<<<1, SBR_BLOCK_MAX, 0, (hipStream_t)stream>>>((const float*)workspace, n_slabs, f,
                                                                       [=] __device__(int j, float acc) { res[j] = sqrtf(acc); });
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}
