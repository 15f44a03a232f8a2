// RBMF, representative-based matrix factorisation (algorithms/mf_algs.py:145-211; Liu et al., RecSys 2011): the r rows of the left
// singular vectors U [n, r], 1 <= r <= 128, whose r x r submatrix has locally maximal volume (maxvol: Goreinov, Oseledets, Savostyanov,
// Tyrtyshnikov and Zamarashkin 2010, where the reference calls maxvolpy), and the closed-form ridge solve behind them.
//   sbr_maxvol_lu_step_f32    step k of the row-pivoted LU of a tall matrix, in place: the pivot rows are maxvol's start
//   sbr_tri_solve_rows_f32    out[i, :] = in[i, :] T^-1, T triangular in LDS: B = L L_top^-1 = U inv(U[idx]), and the ridge solve
//   sbr_maxvol_swap_step_f32  one iteration of the swap loop on B: the largest |B_ij| > tol puts row i in place of basis row j
//   sbr_chol_f32              K = R R^T for an r x r SPD matrix by one workgroup (block128.h, the factorisation of als.hip)
// The two chains are sequences of launches: a launch leaves one candidate per row slab for the next one's arg-max, every workgroup of
// the next launch reduces all of them again and so names the same pivot, and no workgroup ever waits for another inside a kernel.
// fp32, no float atomics, a fixed operation order per element; every arg-max takes the lowest (row, then column) index on a tie: the
// same bits on every run, for every slab size, valid in deterministic mode. tests/rbmf_ref.py restates the algorithm in numpy.
#include "block128.h"

#define RBMF_THREADS 256              // 128 columns x 2 rows at a time; also the width of the block arg-max
#define RBMF_SLAB 256                 // rows per workgroup (slab) unless the caller names another
#define RBMF_SLAB_MAX 1024
#define RBMF_EPS 5.9604645e-8f        // 2^-24

// (v, row, col) beats (bv, brow, bcol): the larger magnitude, then the lower row, then the lower column; a NaN never wins, and an empty
// slab's (-1, -1, -1) loses to every real candidate
__device__ __forceinline__ bool mv_better(float v, int row, int col, float bv, int brow, int bcol) {
  return v > bv || (v == bv && (row < brow || (row == brow && col < bcol)));
}

// the workgroup's best candidate, in sv[0], sr[0], sc[0] for every thread (256 threads; a total order, so the tree's shape is immaterial)
__device__ __forceinline__ void mv_block_best(float v, int row, int col, float* sv, int* sr, int* sc) {
  const int t = threadIdx.x;
  sv[t] = v; sr[t] = row; sc[t] = col;
  __syncthreads();
  for (int w = RBMF_THREADS / 2; w > 0; w >>= 1) {
    if (t < w && mv_better(sv[t + w], sr[t + w], sc[t + w], sv[t], sr[t], sc[t])) {
      sv[t] = sv[t + w]; sr[t] = sr[t + w]; sc[t] = sc[t + w];
    }
    __syncthreads();
  }
}

// the previous launch's candidates, one per slab, reduced by every workgroup alike
__device__ __forceinline__ void mv_reduce_slabs(const float* cv, const int* cr, const int* cc, int n_slabs, float* sv, int* sr, int* sc) {
  float bv = -1.f;
  int br = -1, bc = -1;
  for (int s = threadIdx.x; s < n_slabs; s += RBMF_THREADS) {
    const float v = cv[s];
    const int row = cr[s], col = cc ? cc[s] : 0;
    if (row >= 0 && mv_better(v, row, col, bv, br, bc)) { bv = v; br = row; bc = col; }
  }
  mv_block_best(bv, br, bc, sv, sr, sc);
}

// workspace (four-byte words), S = n_slabs: cand_v [2][S] fp32 | cand_row [2][S] | cand_col [2][S] | pos [n] | maxpiv [1] fp32 | 3 spare
struct mv_ws {
  float* cv; int* cr; int* cc; int* pos; float* maxpiv;
};
static inline int mv_slab(int slab_rows) { return slab_rows > 0 ? slab_rows : RBMF_SLAB; }
static inline mv_ws mv_carve(void* workspace, long n, long S) {
  mv_ws w;
  w.cv = (float*)workspace;
  w.cr = (int*)workspace + 2 * S;
  w.cc = (int*)workspace + 4 * S;
  w.pos = (int*)workspace + 6 * S;
  w.maxpiv = (float*)workspace + 6 * S + n;
  return w;
}

extern "C" long sbr_maxvol_f32_workspace(long n, int slab_rows) {
  if (n < 1 || n > 2147483646L || slab_rows < 0 || slab_rows > RBMF_SLAB_MAX) return 0;
  return 4 * (6 * sbr_slabs(n, mv_slab(slab_rows)) + n + 4);
}

// ---- the row-pivoted LU of A [n, r], one launch per step ------------------------------------------------------------------------------
// pos[m] = -1: row m is not chosen yet; = s: it is the pivot row of step s
__global__ __launch_bounds__(RBMF_THREADS) void maxvol_lu_init_kernel(const float* __restrict__ A, long n, long lda, int slab, int n_slabs,
                                                                      mv_ws w) {
  __shared__ float sv[RBMF_THREADS];
  __shared__ int sr[RBMF_THREADS], sc[RBMF_THREADS];
  const long lo = (long)blockIdx.x * slab;
  const int rows = n - lo < slab ? (int)(n - lo) : slab;
  float bv = -1.f;
  int br = -1;
  for (int q = threadIdx.x; q < rows; q += RBMF_THREADS) {
    w.pos[lo + q] = -1;
    const float v = fabsf(A[(lo + q) * lda]);
    if (mv_better(v, (int)(lo + q), 0, bv, br, 0)) { bv = v; br = (int)(lo + q); }
  }
  mv_block_best(bv, br, 0, sv, sr, sc);
  if (threadIdx.x == 0) {
    w.cv[blockIdx.x] = sv[0];
    w.cr[blockIdx.x] = sr[0];
    if (blockIdx.x == 0) *w.maxpiv = 0.f;
  }
}

__global__ __launch_bounds__(RBMF_THREADS) void maxvol_lu_step_kernel(float* A, long n, long lda, int r, int k, int slab, int n_slabs,
                                                                      int* __restrict__ idx, int* __restrict__ info, mv_ws w) {
#pragma clang fp contract(off)
  __shared__ float sv[RBMF_THREADS];
  __shared__ int sr[RBMF_THREADS], sc[RBMF_THREADS];
  __shared__ float prow[SBR_BLOCK_MAX];
  __shared__ float lrow[RBMF_SLAB_MAX], cabs[RBMF_SLAB_MAX];
  __shared__ int act[RBMF_SLAB_MAX];
  const int t = threadIdx.x, cur = (k & 1) * n_slabs, nxt = ((k + 1) & 1) * n_slabs;
  mv_reduce_slabs(w.cv + cur, w.cr + cur, nullptr, n_slabs, sv, sr, sc);
  const long piv = sr[0];
  __syncthreads();
  if (piv < 0 || piv >= n) {                                        // no finite candidate (NaNs): the same for every workgroup
    if (t == 0) {
      w.cv[nxt + blockIdx.x] = -1.f;
      w.cr[nxt + blockIdx.x] = -1;
      if (blockIdx.x == 0) {
        idx[k] = 0;
        sbr_report_first(info, k + 1);
      }
    }
    return;
  }
  // the pivot row is up to date: it took part, as a row not yet chosen, in every step before this one; nobody writes it in this launch
  for (int j = t; j < r; j += RBMF_THREADS) prow[j] = A[piv * lda + j];
  __syncthreads();
  const float pkk = prow[k];
  if (blockIdx.x == 0 && t == 0) {
    const float largest = *w.maxpiv, mag = fabsf(pkk);
    idx[k] = (int)piv;
    if (!(mag > 0.f && mag > (float)r * RBMF_EPS * largest)) sbr_report_first(info, k + 1);
    *w.maxpiv = fmaxf(largest, mag);
  }
  const long lo = (long)blockIdx.x * slab;
  const int rows = n - lo < slab ? (int)(n - lo) : slab;
  for (int q = t; q < rows; q += RBMF_THREADS) {
    const long m = lo + q;
    const bool on = w.pos[m] < 0 && m != piv;
    if (m == piv) w.pos[m] = k;
    act[q] = on ? 1 : 0;
    lrow[q] = on ? A[m * lda + k] / pkk : 0.f;
    cabs[q] = -1.f;
  }
  __syncthreads();
  const int col = t & (SBR_BLOCK_MAX - 1);
  for (int q = t >> 7; q < rows; q += RBMF_THREADS / SBR_BLOCK_MAX) {
    if (!act[q] || col < k || col >= r) continue;
    float* a = A + (lo + q) * lda + col;
    const float l = lrow[q];
    if (col == k) {
      *a = l;
    } else {
      const float v = fmaf(-l, prow[col], *a);
      *a = v;
      if (col == k + 1) cabs[q] = fabsf(v);
    }
  }
  __syncthreads();
  float bv = -1.f;
  int br = -1;
  for (int q = t; q < rows; q += RBMF_THREADS)
    if (act[q] && mv_better(cabs[q], (int)(lo + q), 0, bv, br, 0)) { bv = cabs[q]; br = (int)(lo + q); }
  mv_block_best(bv, br, 0, sv, sr, sc);
  if (t == 0) {
    w.cv[nxt + blockIdx.x] = sv[0];
    w.cr[nxt + blockIdx.x] = sr[0];
  }
}

// after the last step: a pivot row holds its multipliers in front of the diagonal and its row of the upper factor from there on; the
// upper part goes to Utop (when asked for), the row becomes its row of the unit lower factor L, and that row goes to Ltop
__global__ __launch_bounds__(RBMF_THREADS) void maxvol_lu_unpack_kernel(float* A, long n, long lda, int r, int slab, float* __restrict__ Ltop,
                                                                        long ldl, float* __restrict__ Utop, long ldu, mv_ws w) {
  const long lo = (long)blockIdx.x * slab;
  const int rows = n - lo < slab ? (int)(n - lo) : slab;
  const int col = threadIdx.x & (SBR_BLOCK_MAX - 1);
  if (col >= r) return;
  for (int q = threadIdx.x >> 7; q < rows; q += RBMF_THREADS / SBR_BLOCK_MAX) {
    const int s = w.pos[lo + q];
    if (s < 0 || s >= r) continue;
    float* a = A + (lo + q) * lda + col;
    const float v = *a;
    if (Utop) Utop[(long)s * ldu + col] = col >= s ? v : 0.f;
    const float l = col < s ? v : (col == s ? 1.f : 0.f);
    if (col >= s) *a = l;
    Ltop[(long)s * ldl + col] = l;
  }
}

static int mv_check(const char* who, long n, long ld, int r, const void* ws, long ws_bytes, int slab_rows) {
  SBR_REQUIRE_WIDTH(who, "r", r);
  SBR_REQUIRE(n >= r && n <= 2147483646L, "%s: n=%ld outside [r=%d, 2^31 - 2]", who, n, r);
  SBR_TRY(sbr_check_ld(who, "r", r, {{"ld", ld}}));
  SBR_REQUIRE(slab_rows >= 0 && slab_rows <= RBMF_SLAB_MAX, "%s: slab_rows=%d outside [0, %d]", who, slab_rows, RBMF_SLAB_MAX);
  SBR_REQUIRE_WORKSPACE(who, ws, ws_bytes, sbr_maxvol_f32_workspace(n, slab_rows), 4);
  return SBR_OK;
}

extern "C" int sbr_maxvol_lu_step_f32(float* A, long n, long lda, int r, int k, int* idx, float* Ltop, long ldl, float* Utop, long ldu, int* info,
                                      void* workspace, long workspace_bytes, int slab_rows, void* stream) {
  SBR_TRY(mv_check(__func__, n, lda, r, workspace, workspace_bytes, slab_rows));
  SBR_REQUIRE(k >= 0 && k < r, "%s: step k=%d outside [0, r=%d)", __func__, k, r);
  SBR_TRY(sbr_check_ld(__func__, "r", r, {{"ldl", ldl}, {"ldu", Utop ? ldu : r}}));
  SBR_REQUIRE_OPERANDS(__func__, A && idx && Ltop && info);
  const int slab = mv_slab(slab_rows), S = (int)sbr_slabs(n, mv_slab(slab_rows));
  const mv_ws w = mv_carve(workspace, n, S);
  hipStream_t st = (hipStream_t)stream;
  if (k == 0) {
    maxvol_lu_init_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(A, n, lda, slab, S, w);
    SBR_CHECK_LAUNCH(__func__);
  }
  maxvol_lu_step_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(A, n, lda, r, k, slab, S, idx, info, w);
  SBR_CHECK_LAUNCH(__func__);
  if (k == r - 1) {
    maxvol_lu_unpack_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(A, n, lda, r, slab, Ltop, ldl, Utop, ldu, w);
    SBR_CHECK_LAUNCH(__func__);
  }
  return SBR_OK;
}

// ---- out[i, :] = in[i, :] T^-1 ------------------------------------------------------------------------------------------------------
// T [r][ld] in LDS once per workgroup (block128.h: sbr_stage_triangle); a wave owns a row of `in` (SbrRow2). x T = b by columns: lower T,
// j descending: x_j = b_j / T_jj, then b_m <- fmaf(-x_j, T[j][m], b_m) for m < j; upper T: j ascending, m > j. Row j of T is read along
// the lanes: no bank twice.
#define TRI_WAVES (RBMF_THREADS / 64)
#define TRI_MAX_BLOCKS 1024
static inline size_t tri_lds_bytes(int r) { return 4 * sbr_odd_cells(r, r); }

__global__ __launch_bounds__(RBMF_THREADS) void tri_solve_rows_kernel(const float* in, long ldi, long n, int r, const float* __restrict__ T,
                                                                      long ldt, int upper, int unit, float* out, long ldo) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float tri_lds[];
  const int ld = sbr_odd_ld(r), t = threadIdx.x;
  sbr_stage_triangle(tri_lds, T, ldt, r, upper, t, RBMF_THREADS);
  __syncthreads();
  const SbrRow2 w(r);
  for (long row = (long)blockIdx.x * TRI_WAVES + (t >> 6); row < n; row += (long)gridDim.x * TRI_WAVES) {
    float b0, b1;
    w.load(in + row * ldi, b0, b1);
    for (int s = 0; s < r; ++s) {
      const int j = upper ? s : r - 1 - s;
      const float* tj = tri_lds + j * ld;
      float xj = __shfl(j < 64 ? b0 : b1, j & 63, 64);
      if (!unit) xj = xj / tj[j];
      if (j < 64) { if (w.lane == j) b0 = xj; } else { if (w.lane == j - 64) b1 = xj; }
      const bool u0 = upper ? w.lane > j : w.lane < j, u1 = upper ? w.lane + 64 > j : w.lane + 64 < j;
      if (w.h0 && u0) b0 = fmaf(-xj, tj[w.lane], b0);
      if (w.h1 && u1) b1 = fmaf(-xj, tj[w.lane + 64], b1);
    }
    w.store(out + row * ldo, b0, b1);
  }
}

extern "C" int sbr_tri_solve_rows_f32(const float* in, long ldi, long n, int r, const float* T, long ldt, int upper, int unit, float* out, long ldo,
                                      void* stream) {
  SBR_REQUIRE_WIDTH(__func__, "r", r);
  SBR_REQUIRE(n >= 0 && n <= 2147483646L, "%s: n=%ld outside [0, 2^31 - 2]", __func__, n);
  SBR_TRY(sbr_check_ld(__func__, "r", r, {{"ldi", ldi}, {"ldt", ldt}, {"ldo", ldo}}));
  SBR_REQUIRE((upper == 0 || upper == 1) && (unit == 0 || unit == 1), "%s: flags upper=%d unit=%d are not 0 / 1", __func__, upper, unit);
  if (n == 0) return SBR_OK;
  SBR_REQUIRE_OPERANDS(__func__, in && T && out);
  SBR_RAISE_LDS(tri_solve_rows_kernel, tri_lds_bytes(SBR_BLOCK_MAX));
  const long blocks = sbr_slabs(n, TRI_WAVES);
  tri_solve_rows_kernel<<<(unsigned)(blocks < TRI_MAX_BLOCKS ? blocks : TRI_MAX_BLOCKS), RBMF_THREADS, tri_lds_bytes(r), (hipStream_t)stream>>>(
      in, ldi, n, r, T, ldt, upper, unit, out, ldo);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}

// ---- the swap loop on B [n, r] = U inv(U[idx]), one launch per iteration ----------------------------------------------------------------
// pos[m] = c: row m is basis row c (idx[c] = m) and stands for e_c: what memory holds of it is never read again; pos[m] = -1 otherwise.
__global__ __launch_bounds__(RBMF_THREADS) void maxvol_swap_init_kernel(const float* __restrict__ B, long n, long ldb, int r, int slab, int n_slabs,
                                                                        const int* __restrict__ idx, mv_ws w) {
  __shared__ float sv[RBMF_THREADS];
  __shared__ int sr[RBMF_THREADS], sc[RBMF_THREADS];
  __shared__ int basis[SBR_BLOCK_MAX];
  __shared__ int ps[RBMF_SLAB_MAX];
  const int t = threadIdx.x;
  if (t < r) basis[t] = idx[t];
  __syncthreads();
  const long lo = (long)blockIdx.x * slab;
  const int rows = n - lo < slab ? (int)(n - lo) : slab;
  for (int q = t; q < rows; q += RBMF_THREADS) {
    int p = -1;
    for (int c = 0; c < r; ++c)
      if (basis[c] == (int)(lo + q)) p = c;
    ps[q] = p;
    w.pos[lo + q] = p;
  }
  __syncthreads();
  const int col = t & (SBR_BLOCK_MAX - 1);
  float bv = -1.f;
  int br = -1;
  if (col < r)
    for (int q = t >> 7; q < rows; q += RBMF_THREADS / SBR_BLOCK_MAX) {
      if (ps[q] >= 0) continue;
      const float v = fabsf(B[(lo + q) * ldb + col]);
      if (v > bv) { bv = v; br = (int)(lo + q); }                    // rows ascending: the lowest row of a tie stays
    }
  mv_block_best(bv, br, br < 0 ? -1 : col, sv, sr, sc);
  if (t == 0) {
    w.cv[blockIdx.x] = sv[0];
    w.cr[blockIdx.x] = sr[0];
    w.cc[blockIdx.x] = sc[0];
  }
}

__global__ __launch_bounds__(RBMF_THREADS) void maxvol_swap_step_kernel(float* B, long n, long ldb, int r, float tol, int s, int slab, int n_slabs,
                                                                        int* __restrict__ idx, int* __restrict__ n_swaps, mv_ws w) {
#pragma clang fp contract(off)
  __shared__ float sv[RBMF_THREADS];
  __shared__ int sr[RBMF_THREADS], sc[RBMF_THREADS];
  __shared__ float wrow[SBR_BLOCK_MAX];
  __shared__ float bm[RBMF_SLAB_MAX];
  __shared__ int role[RBMF_SLAB_MAX];                               // 0: left alone | 1: an ordinary row | 2: the row that leaves the basis
  const int t = threadIdx.x, cur = (s & 1) * n_slabs, nxt = ((s + 1) & 1) * n_slabs;
  mv_reduce_slabs(w.cv + cur, w.cr + cur, w.cc + cur, n_slabs, sv, sr, sc);
  const float top = sv[0];
  const long i = sr[0];
  const int j = sc[0];
  __syncthreads();
  if (!(top > tol) || i < 0 || i >= n || j < 0 || j >= r) {           // converged: B is not touched, the candidates move on as they are
    if (t == 0) {
      w.cv[nxt + blockIdx.x] = w.cv[cur + blockIdx.x];
      w.cr[nxt + blockIdx.x] = w.cr[cur + blockIdx.x];
      w.cc[nxt + blockIdx.x] = w.cc[cur + blockIdx.x];
    }
    return;
  }
  // row i enters the basis in place of row idx[j]. Nobody writes row i in this launch (it stands for e_j from now on), so every
  // workgroup reads the same w = (B[i, :] - e_j) / B_ij
  const float bij = B[i * ldb + j];
  if (t < r) wrow[t] = (B[i * ldb + t] - (t == j ? 1.f : 0.f)) / bij;
  if (blockIdx.x == 0 && t == 0) {
    idx[j] = (int)i;
    *n_swaps = *n_swaps + 1;
  }
  const long lo = (long)blockIdx.x * slab;
  const int rows = n - lo < slab ? (int)(n - lo) : slab;
  for (int q = t; q < rows; q += RBMF_THREADS) {
    const long m = lo + q;
    const int p = w.pos[m];
    int ro = 0;
    float b = 0.f;
    if (m == i) {
      w.pos[m] = j;
    } else if (p == j) {
      ro = 2; b = 1.f;                                              // it was e_j
      w.pos[m] = -1;
    } else if (p < 0) {
      ro = 1; b = B[m * ldb + j];
    }
    role[q] = ro;
    bm[q] = b;
  }
  __syncthreads();
  const int col = t & (SBR_BLOCK_MAX - 1);
  float bv = -1.f;
  int br = -1;
  if (col < r)
    for (int q = t >> 7; q < rows; q += RBMF_THREADS / SBR_BLOCK_MAX) {
      const int ro = role[q];
      if (!ro) continue;
      float* a = B + (lo + q) * ldb + col;
      const float v = fmaf(-bm[q], wrow[col], ro == 2 ? (col == j ? 1.f : 0.f) : *a);
      *a = v;
      if (fabsf(v) > bv) { bv = fabsf(v); br = (int)(lo + q); }
    }
  mv_block_best(bv, br, br < 0 ? -1 : col, sv, sr, sc);
  if (t == 0) {
    w.cv[nxt + blockIdx.x] = sv[0];
    w.cr[nxt + blockIdx.x] = sr[0];
    w.cc[nxt + blockIdx.x] = sc[0];
  }
}

extern "C" int sbr_maxvol_swap_step_f32(float* B, long n, long ldb, int r, float tol, int s, int* idx, int* n_swaps, void* workspace,
                                        long workspace_bytes, int slab_rows, void* stream) {
  SBR_TRY(mv_check(__func__, n, ldb, r, workspace, workspace_bytes, slab_rows));
  SBR_REQUIRE(tol >= 1.f && sbr_pos_finite(tol), "%s: tol=%g is not a finite number >= 1", __func__, (double)tol);
  SBR_REQUIRE(s >= 0, "%s: step s=%d is negative", __func__, s);
  SBR_REQUIRE_OPERANDS(__func__, B && idx && n_swaps);
  const int slab = mv_slab(slab_rows), S = (int)sbr_slabs(n, mv_slab(slab_rows));
  const mv_ws w = mv_carve(workspace, n, S);
  hipStream_t st = (hipStream_t)stream;
  if (s == 0) {
    maxvol_swap_init_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(B, n, ldb, r, slab, S, idx, w);
    SBR_CHECK_LAUNCH(__func__);
  }
  maxvol_swap_step_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(B, n, ldb, r, tol, s, slab, S, idx, n_swaps, w);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}

// ---- K = R R^T, one workgroup ---------------------------------------------------------------------------------------------------------
static inline size_t chol_lds_bytes(int n) { return 4 * (sbr_odd_cells(n, n) + SBR_BLOCK_MAX); }

__global__ __launch_bounds__(SBR_BLOCK_MAX) void chol_kernel(const float* __restrict__ K, int n, long ldk, float* __restrict__ R, long ldr,
                                                          int* __restrict__ info) {
  extern __shared__ __align__(16) float chol_lds[];
  const int lda = sbr_odd_ld(n), t = threadIdx.x;
  float* diag = chol_lds;
  float* A = diag + SBR_BLOCK_MAX;
  sbr_stage_triangle(A, K, ldk, n, 0, t, SBR_BLOCK_MAX);              // the lower triangle is read
  __syncthreads();
  sbr_chol_lds(A, lda, n, n, diag, t, [=](int p) { sbr_report_first(info, p + 1); });
  for (int e = t; e < n * n; e += SBR_BLOCK_MAX) {
    const int i = e / n, j = e - i * n;
    R[(long)i * ldr + j] = j < i ? A[i * lda + j] : (j == i ? diag[i] : 0.f);
  }
}

extern "C" int sbr_chol_f32(const float* K, int n, long ldk, float* R, long ldr, int* info, void* stream) {
  SBR_REQUIRE_WIDTH(__func__, "n", n);
  SBR_TRY(sbr_check_ld(__func__, "n", n, {{"ldk", ldk}, {"ldr", ldr}}));
  SBR_REQUIRE_OPERANDS(__func__, K && R && info);
  SBR_RAISE_LDS(chol_kernel, chol_lds_bytes(SBR_BLOCK_MAX));
  chol_kernel<<<1, SBR_BLOCK_MAX, chol_lds_bytes(n), (hipStream_t)stream>>>(K, n, ldk, R, ldr, info);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}
