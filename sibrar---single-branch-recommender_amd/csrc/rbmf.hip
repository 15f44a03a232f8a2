// RBMF, representative-based matrix factorisation (algorithms/mf_algs.py:145-211; Liu et al., RecSys 2011): the r rows of the left
// singular vectors U [n, r], 1 <= r <= 128, whose r x r submatrix has locally maximal volume (maxvol: Goreinov, Oseledets, Savostyanov,
// Tyrtyshnikov and Zamarashkin 2010, where the reference calls maxvolpy), and the closed-form ridge solve behind them.
//   sbr_maxvol_lu_step_f32    step k of the row-pivoted LU of a tall matrix, in place: the pivot rows are maxvol's start
//   sbr_tri_solve_rows_f32    out[i, :] = in[i, :] T^-1, T triangular in LDS: B = L L_top^-1 = U inv(U[idx]), and the ridge solve
//   sbr_maxvol_swap_step_f32  one iteration of the swap loop on B: the largest |B_ij| > tol puts row i in place of basis row j
//   sbr_chol_f32              K = R R^T for an r x r SPD matrix by one workgroup (chol_lds.h, the factorisation of als.hip)
// The two chains are sequences of launches: a launch leaves one candidate per row slab for the next one's arg-max, every workgroup of
// the next launch reduces all of them again and so names the same pivot, and no workgroup ever waits for another inside a kernel.
// fp32, no float atomics, a fixed operation order per element; every arg-max takes the lowest (row, then column) index on a tie: the
// same bits on every run, for every slab size, valid in deterministic mode. tests/rbmf_ref.py restates the algorithm in numpy.
#include "common.h"
#include "chol_lds.h"

#define RBMF_R_MAX 128
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
static inline long mv_slabs(long n, int slab_rows) { return (n + mv_slab(slab_rows) - 1) / mv_slab(slab_rows); }
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
  return 4 * (6 * mv_slabs(n, slab_rows) + n + 4);
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
  __shared__ float prow[RBMF_R_MAX];
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
        if (*info == 0) *info = k + 1;
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
    if (!(mag > 0.f && mag > (float)r * RBMF_EPS * largest) && *info == 0) *info = k + 1;
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
  const int col = t & (RBMF_R_MAX - 1);
  for (int q = t >> 7; q < rows; q += RBMF_THREADS / RBMF_R_MAX) {
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
  const int col = threadIdx.x & (RBMF_R_MAX - 1);
  if (col >= r) return;
  for (int q = threadIdx.x >> 7; q < rows; q += RBMF_THREADS / RBMF_R_MAX) {
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
  SBR_REQUIRE(r >= 1 && r <= RBMF_R_MAX, "%s: r=%d outside [1, %d]", who, r, RBMF_R_MAX);
  SBR_REQUIRE(n >= r && n <= 2147483646L, "%s: n=%ld outside [r=%d, 2^31 - 2]", who, n, r);
  SBR_REQUIRE(ld >= r, "%s: leading dimension %ld below r=%d", who, ld, r);
  SBR_REQUIRE(slab_rows >= 0 && slab_rows <= RBMF_SLAB_MAX, "%s: slab_rows=%d outside [0, %d]", who, slab_rows, RBMF_SLAB_MAX);
  const long need = sbr_maxvol_f32_workspace(n, slab_rows);
  SBR_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 3) == 0, "%s: workspace of %ld bytes, %ld needed", who, ws_bytes, need);
  return SBR_OK;
}

extern "C" int sbr_maxvol_lu_step_f32(float* A, long n, long lda, int r, int k, int* idx, float* Ltop, long ldl, float* Utop, long ldu, int* info,
                                      void* workspace, long workspace_bytes, int slab_rows, void* stream) {
  const char* who = "sbr_maxvol_lu_step_f32";
  if (int rc = mv_check(who, n, lda, r, workspace, workspace_bytes, slab_rows)) return rc;
  SBR_REQUIRE(k >= 0 && k < r, "%s: step k=%d outside [0, r=%d)", who, k, r);
  SBR_REQUIRE(ldl >= r && (!Utop || ldu >= r), "%s: leading dimension below r=%d (ldl=%ld, ldu=%ld)", who, r, ldl, ldu);
  SBR_REQUIRE(A && idx && Ltop && info, "%s: null operand", who);
  const int slab = mv_slab(slab_rows), S = (int)mv_slabs(n, slab_rows);
  const mv_ws w = mv_carve(workspace, n, S);
  hipStream_t st = (hipStream_t)stream;
  if (k == 0) {
    maxvol_lu_init_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(A, n, lda, slab, S, w);
    SBR_CHECK_LAUNCH(who);
  }
  maxvol_lu_step_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(A, n, lda, r, k, slab, S, idx, info, w);
  SBR_CHECK_LAUNCH(who);
  if (k == r - 1) {
    maxvol_lu_unpack_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(A, n, lda, r, slab, Ltop, ldl, Utop, ldu, w);
    SBR_CHECK_LAUNCH(who);
  }
  return SBR_OK;
}

// ---- out[i, :] = in[i, :] T^-1 ------------------------------------------------------------------------------------------------------
// T [r][ld] in LDS once per workgroup; a wave owns a row of `in`, lane l holds its elements l and l + 64. x T = b by columns: lower T,
// j descending: x_j = b_j / T_jj, then b_m <- fmaf(-x_j, T[j][m], b_m) for m < j; upper T: j ascending, m > j. Row j of T is read along
// the lanes: no bank twice.
#define TRI_WAVES (RBMF_THREADS / 64)
#define TRI_MAX_BLOCKS 1024
static inline size_t tri_lds_bytes(int r) { return 4 * (size_t)r * sbr_chol_lda(r); }

__global__ __launch_bounds__(RBMF_THREADS) void tri_solve_rows_kernel(const float* in, long ldi, long n, int r, const float* __restrict__ T,
                                                                      long ldt, int upper, int unit, float* out, long ldo) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float tri_lds[];
  const int ld = sbr_chol_lda(r), t = threadIdx.x, lane = t & 63;
  for (int e = t; e < r * r; e += RBMF_THREADS) {
    const int i = e / r, j = e - i * r;
    tri_lds[i * ld + j] = (upper ? j >= i : j <= i) ? T[(long)i * ldt + j] : 0.f;       // only the triangle is read
  }
  __syncthreads();
  const bool h0 = lane < r, h1 = lane + 64 < r;
  for (long row = (long)blockIdx.x * TRI_WAVES + (t >> 6); row < n; row += (long)gridDim.x * TRI_WAVES) {
    float b0 = h0 ? in[row * ldi + lane] : 0.f, b1 = h1 ? in[row * ldi + lane + 64] : 0.f;
    for (int s = 0; s < r; ++s) {
      const int j = upper ? s : r - 1 - s;
      const float* tj = tri_lds + j * ld;
      float xj = __shfl(j < 64 ? b0 : b1, j & 63, 64);
      if (!unit) xj = xj / tj[j];
      if (j < 64) { if (lane == j) b0 = xj; } else { if (lane == j - 64) b1 = xj; }
      const bool u0 = upper ? lane > j : lane < j, u1 = upper ? lane + 64 > j : lane + 64 < j;
      if (h0 && u0) b0 = fmaf(-xj, tj[lane], b0);
      if (h1 && u1) b1 = fmaf(-xj, tj[lane + 64], b1);
    }
    if (h0) out[row * ldo + lane] = b0;
    if (h1) out[row * ldo + lane + 64] = b1;
  }
}

extern "C" int sbr_tri_solve_rows_f32(const float* in, long ldi, long n, int r, const float* T, long ldt, int upper, int unit, float* out, long ldo,
                                      void* stream) {
  const char* who = "sbr_tri_solve_rows_f32";
  SBR_REQUIRE(r >= 1 && r <= RBMF_R_MAX, "%s: r=%d outside [1, %d]", who, r, RBMF_R_MAX);
  SBR_REQUIRE(n >= 0 && n <= 2147483646L, "%s: n=%ld outside [0, 2^31 - 2]", who, n);
  SBR_REQUIRE(ldi >= r && ldt >= r && ldo >= r, "%s: leading dimension below r=%d (ldi=%ld, ldt=%ld, ldo=%ld)", who, r, ldi, ldt, ldo);
  SBR_REQUIRE((upper == 0 || upper == 1) && (unit == 0 || unit == 1), "%s: flags upper=%d unit=%d are not 0 / 1", who, upper, unit);
  if (n == 0) return SBR_OK;
  SBR_REQUIRE(in && T && out, "%s: null operand", who);
  static SbrLdsSlot lds_slot;
  const int lds_rc = sbr_raise_lds(who, (const void*)tri_solve_rows_kernel, &lds_slot, tri_lds_bytes(RBMF_R_MAX));
  if (lds_rc) return lds_rc;
  const long blocks = (n + TRI_WAVES - 1) / TRI_WAVES;
  tri_solve_rows_kernel<<<(unsigned)(blocks < TRI_MAX_BLOCKS ? blocks : TRI_MAX_BLOCKS), RBMF_THREADS, tri_lds_bytes(r), (hipStream_t)stream>>>(
      in, ldi, n, r, T, ldt, upper, unit, out, ldo);
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}

// ---- the swap loop on B [n, r] = U inv(U[idx]), one launch per iteration ----------------------------------------------------------------
// pos[m] = c: row m is basis row c (idx[c] = m) and stands for e_c: what memory holds of it is never read again; pos[m] = -1 otherwise.
__global__ __launch_bounds__(RBMF_THREADS) void maxvol_swap_init_kernel(const float* __restrict__ B, long n, long ldb, int r, int slab, int n_slabs,
                                                                        const int* __restrict__ idx, mv_ws w) {
  __shared__ float sv[RBMF_THREADS];
  __shared__ int sr[RBMF_THREADS], sc[RBMF_THREADS];
  __shared__ int basis[RBMF_R_MAX];
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
  const int col = t & (RBMF_R_MAX - 1);
  float bv = -1.f;
  int br = -1;
  if (col < r)
    for (int q = t >> 7; q < rows; q += RBMF_THREADS / RBMF_R_MAX) {
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
  __shared__ float wrow[RBMF_R_MAX];
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
  const int col = t & (RBMF_R_MAX - 1);
  float bv = -1.f;
  int br = -1;
  if (col < r)
    for (int q = t >> 7; q < rows; q += RBMF_THREADS / RBMF_R_MAX) {
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
  const char* who = "sbr_maxvol_swap_step_f32";
  if (int rc = mv_check(who, n, ldb, r, workspace, workspace_bytes, slab_rows)) return rc;
  SBR_REQUIRE(tol >= 1.f && sbr_pos_finite(tol), "%s: tol=%g is not a finite number >= 1", who, (double)tol);
  SBR_REQUIRE(s >= 0, "%s: step s=%d is negative", who, s);
  SBR_REQUIRE(B && idx && n_swaps, "%s: null operand", who);
  const int slab = mv_slab(slab_rows), S = (int)mv_slabs(n, slab_rows);
  const mv_ws w = mv_carve(workspace, n, S);
  hipStream_t st = (hipStream_t)stream;
  if (s == 0) {
    maxvol_swap_init_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(B, n, ldb, r, slab, S, idx, w);
    SBR_CHECK_LAUNCH(who);
  }
  maxvol_swap_step_kernel<<<(unsigned)S, RBMF_THREADS, 0, st>>>(B, n, ldb, r, tol, s, slab, S, idx, n_swaps, w);
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}

// ---- K = R R^T, one workgroup ---------------------------------------------------------------------------------------------------------
static inline size_t chol_lds_bytes(int n) { return 4 * ((size_t)n * sbr_chol_lda(n) + RBMF_R_MAX); }

__global__ __launch_bounds__(RBMF_R_MAX) void chol_kernel(const float* __restrict__ K, int n, long ldk, float* __restrict__ R, long ldr,
                                                          int* __restrict__ info) {
  extern __shared__ __align__(16) float chol_lds[];
  const int lda = sbr_chol_lda(n), t = threadIdx.x;
  float* diag = chol_lds;
  float* A = diag + RBMF_R_MAX;
  for (int e = t; e < n * n; e += RBMF_R_MAX) {
    const int i = e / n, j = e - i * n;
    A[i * lda + j] = j <= i ? K[(long)i * ldk + j] : 0.f;            // the lower triangle is read
  }
  __syncthreads();
  sbr_chol_lds(A, lda, n, n, diag, t, [=](int p) { atomicCAS(info, 0, p + 1); });
  for (int e = t; e < n * n; e += RBMF_R_MAX) {
    const int i = e / n, j = e - i * n;
    R[(long)i * ldr + j] = j < i ? A[i * lda + j] : (j == i ? diag[i] : 0.f);
  }
}

extern "C" int sbr_chol_f32(const float* K, int n, long ldk, float* R, long ldr, int* info, void* stream) {
  const char* who = "sbr_chol_f32";
  SBR_REQUIRE(n >= 1 && n <= RBMF_R_MAX, "%s: n=%d outside [1, %d]", who, n, RBMF_R_MAX);
  SBR_REQUIRE(ldk >= n && ldr >= n, "%s: leading dimension below n=%d (ldk=%ld, ldr=%ld)", who, n, ldk, ldr);
  SBR_REQUIRE(K && R && info, "%s: null operand", who);
  static SbrLdsSlot lds_slot;
  const int lds_rc = sbr_raise_lds(who, (const void*)chol_kernel, &lds_slot, chol_lds_bytes(RBMF_R_MAX));
  if (lds_rc) return lds_rc;
  chol_kernel<<<1, RBMF_R_MAX, chol_lds_bytes(n), (hipStream_t)stream>>>(K, n, ldk, R, ldr, info);
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}
