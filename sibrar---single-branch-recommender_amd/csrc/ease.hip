// EASE (algorithms/linear_algs.py:130-175, Steck 2019): item-item weights from the Gram matrix of 0/1 interaction data.
//   sbr_gram_dense        G = X^T X + diag_add I as dense fp32 rows, counted exactly (linear_algs.py:150-153)
//   sbr_spd_inverse_f32   in-place inverse of a symmetric positive definite fp32 matrix by the blocked symmetric sweep (:155)
//   sbr_ease_weights_f32  B[i, j] = P[i, j] / -P[j, j], zero diagonal, in place (:157-158)
// No float atomics anywhere: the counts are integers (LDS integer atomics), every float has one owner per launch and a fixed
// operation order, so all three give the same bits on every run and are valid in deterministic mode.
#include "block128.h"
#include "csr_walk.h"

typedef float ease_f32x16 __attribute__((ext_vector_type(16)));

// ---- Gram matrix ------------------------------------------------------------------------------------------------------------------
#define GRAM_THREADS 1024
#define GRAM_WAVES (GRAM_THREADS / 64)
#define GRAM_N_MAX (1 << 24)         // a count is at most the number of rows of X: converted to fp32 exactly

// One workgroup per row i of G. (indptr, indices) is X^T (row i: the users of item i), (t_indptr, t_indices) is X (a user's items):
// the count of column j is the number of users that have both items. Every element of the row is written, zeros included.
__global__ __launch_bounds__(GRAM_THREADS) void gram_dense_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                                  const long* __restrict__ t_indptr, const int* __restrict__ t_indices,
                                                                  int m, int r0, float diag_add, int tw, float* __restrict__ G, long ld) {
  extern __shared__ unsigned int cnt[];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i = r0 + (int)blockIdx.x;
  const long f_beg = indptr[i], f_end = indptr[i + 1];
  float* row = G + (long)i * ld;
  for (int t0 = 0; t0 < m; t0 += tw) {
    const int t1 = t0 + tw < m ? t0 + tw : m, width = t1 - t0;
    for (int x = t; x < width; x += GRAM_THREADS) cnt[x] = 0u;
    __syncthreads();
    sbr_cooc_count_tile(indices, f_beg, f_end, t_indptr, t_indices, t0, width, w, GRAM_WAVES, lane, cnt);
    __syncthreads();
    for (int x = t; x < width; x += GRAM_THREADS) {
      const float c = (float)cnt[x];
      row[t0 + x] = t0 + x == i ? c + diag_add : c;
    }
    __syncthreads();
  }
}

extern "C" int sbr_gram_dense(const long* indptr, const int* indices, const long* t_indptr, const int* t_indices, int n, int m, int r0,
                              int r1, float diag_add, int tile_cols, float* G, long ld, void* stream) {
  SBR_REQUIRE(n >= 0 && n <= GRAM_N_MAX && m >= 0, "%s: shape [%d, %d] outside [0, 2^24] x [0, 2^31): a column with more than 2^24 entries "
              "has no exact fp32 count", __func__, n, m);
  SBR_REQUIRE_ROWS(__func__, r0, r1, m);
  SBR_TRY(sbr_check_ld(__func__, "m", m, {{"ld", ld}}));
  static SbrLdsSlot lds_slot;
  const int tw = sbr_row_tile(__func__, (const void*)gram_dense_kernel, &lds_slot, m, tile_cols, 0, r1 - r0,
                              indptr && indices && t_indptr && t_indices && G);
  if (tw <= 0) return -tw;
  // the kernel owns X^T's row i: the roles of the matrix and its transpose are those of sbr_knn_topk on X^T
  gram_dense_kernel<<<(unsigned)(r1 - r0), GRAM_THREADS, 4 * (size_t)tw, (hipStream_t)stream>>>(t_indptr, t_indices, indptr, indices, m, r0,
                                                                                         diag_add, tw, G, ld);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}

// ---- SPD inverse: the blocked symmetric sweep ----------------------------------------------------------------------------------------
// Sweeping the pivot block K of a symmetric A (D = A[K, K], J = the other indices) gives
//   A[K, K] <- -D^-1      A[K, J] <- D^-1 A[K, J]      A[J, K] <- (A[K, J] D^-1 ... =) its transpose      A[J, J] <- A[J, J] - A[J, K] D^-1 A[K, J]
// and after every block has been swept once A = -G^-1. Blocks already swept belong to J like the others. Per pivot block, three
// launches: spd_diag_kernel (D^-1), spd_panel_kernel (P = A[K, :], R = D^-1 P), spd_update_kernel (the rank-64 update and the new
// pivot rows and columns). Workspace: [64 x 64 D^-1][64 x ldp P][64 x ldp R], ldp = n rounded up to 128; the rows behind a ragged last
// block and the columns behind n hold zeros, so the update needs no bounds on its operands.
#define SPD_B 64                     // pivot block
#define SPD_T 128                    // tile of the update: 4 waves x (2 x 2) MFMA tiles of 32 x 32
#define SPD_N_MAX (1 << 20)

static inline long spd_ldp(int n) { return ((long)n + SPD_T - 1) / SPD_T * SPD_T; }

// One workgroup: D = A[K, K] (b x b, b <= 64) -> D^-1 by unpivoted Gauss-Jordan in LDS, step p for every (i, j) at once:
//   d = 1 / D[p][p];  D[p][p] = d;  D[p][j] = D[p][j] d;  D[i][p] = -D[i][p] d;  D[i][j] = D[i][j] - D[i][p] (D[p][j] d)    (i, j != p)
// The 64 x 64 result is padded with zeros. info: 1 + the matrix index of the first pivot <= 0 or not finite, kept once set.
__global__ __launch_bounds__(256) void spd_diag_kernel(const float* __restrict__ A, long ld, int k0, int b, float* __restrict__ Dinv,
                                                       int* __restrict__ info) {
  __shared__ float Ds[SPD_B][SPD_B + 1];
  const int t = threadIdx.x, j = t & 63, w = t >> 6;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = w + 4 * q;
    Ds[i][j] = (i < b && j < b) ? A[(long)(k0 + i) * ld + k0 + j] : 0.f;
  }
  __syncthreads();
  int bad = 0;
  for (int p = 0; p < b; ++p) {
    const float piv = Ds[p][p];
    if (bad == 0 && !sbr_pos_finite(piv)) bad = 1 + k0 + p;
    const float d = 1.f / piv;
    const float rp = Ds[p][j] * d;
    float cp[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) cp[q] = Ds[w + 4 * q][p];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = w + 4 * q;
      float v;
      if (i == p) v = j == p ? d : rp;
      else if (j == p) v = -cp[q] * d;
      else v = Ds[i][j] - cp[q] * rp;
      Ds[i][j] = v;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) Dinv[(w + 4 * q) * SPD_B + j] = Ds[w + 4 * q][j];
  if (t == 0 && bad != 0) sbr_report_first(info, bad);
}

// One workgroup per 64 columns of the panel (the grid covers ldp): P = A[K, :] and R = D^-1 P, R[p][j] = fmaf chain over q = 0 .. 63
// ascending from +0; in the pivot columns R holds -D^-1, which is what the update stores there. Zeros behind b and behind n.
__global__ __launch_bounds__(256) void spd_panel_kernel(const float* __restrict__ A, long ld, int n, int k0, int b,
                                                        const float* __restrict__ Dinv, float* __restrict__ P, float* __restrict__ R,
                                                        long ldp) {
  __shared__ float Ds[SPD_B][SPD_B], Ps[SPD_B][SPD_B];
  const int t = threadIdx.x, jj = t & 63, w = t >> 6;
  const int j0 = (int)blockIdx.x * SPD_B, gj = j0 + jj;
  for (int e = t; e < SPD_B * SPD_B; e += 256) Ds[e >> 6][e & 63] = Dinv[e];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int p = w + 4 * q;
    const float v = (p < b && gj < n) ? A[(long)(k0 + p) * ld + gj] : 0.f;
    Ps[p][jj] = v;
    P[(long)p * ldp + gj] = v;
  }
  __syncthreads();
  float r[16];
  if (j0 == k0) {
#pragma unroll
    for (int q = 0; q < 16; ++q) r[q] = -Ds[w + 4 * q][jj];
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) r[q] = 0.f;
    for (int s = 0; s < SPD_B; ++s) {
      const float ps = Ps[s][jj];
#pragma unroll
      for (int q = 0; q < 16; ++q) r[q] = fmaf(Ds[w + 4 * q][s], ps, r[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) R[(long)(w + 4 * q) * ldp + gj] = r[q];
}

// One workgroup per 128 x 128 tile of A, on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: bit for bit an fmaf chain over p ascending):
//   S[i][j] = sum_p P[p][i] R[p][j] from +0, then per element
//   i in K: R[i - k0][j]  (-D^-1 in the pivot columns)     j in K: R[j - k0][i]     otherwise: A[i][j] - S[i][j]
// times sgn (-1 in the last step: the sweep ends at -G^-1). Both operand panels (64 x 128 each) are staged in LDS once; the tile of A
// is fetched under the MFMAs. Two workgroups per CU (64 KiB of LDS each): at most 256 registers per lane.
__global__ __launch_bounds__(256, 2) void spd_update_kernel(float* __restrict__ A, long ld, int n, int k0, const float* __restrict__ P,
                                                         const float* __restrict__ R, long ldp, float sgn) {
  __shared__ __attribute__((aligned(16))) float Ps[SPD_B][SPD_T];
  __shared__ __attribute__((aligned(16))) float Rs[SPD_B][SPD_T];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
  const int i0 = (int)blockIdx.y * SPD_T, j0 = (int)blockIdx.x * SPD_T;
#pragma unroll
  for (int e = t; e < SPD_B * (SPD_T / 4); e += 256) {
    const int p = e >> 5, c = (e & 31) * 4;
    *reinterpret_cast<float4*>(&Ps[p][c]) = *reinterpret_cast<const float4*>(P + (long)p * ldp + i0 + c);
    *reinterpret_cast<float4*>(&Rs[p][c]) = *reinterpret_cast<const float4*>(R + (long)p * ldp + j0 + c);
  }
  __syncthreads();
  const int gj_base = j0 + wn * 64 + l31, gi_base = i0 + wm * 64 + 4 * half;
  float cv[2][2][16];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int gi = gi_base + mi * 32 + (r & 3) + 8 * (r >> 2);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int gj = gj_base + ni * 32;
        cv[mi][ni][r] = (gi < n && gj < n) ? A[(long)gi * ld + gj] : 0.f;
      }
    }
  ease_f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
#pragma unroll 4
  for (int kk = 0; kk < SPD_B; kk += 2) {
    const int k = kk + half;
    const float a0 = Ps[k][wm * 64 + l31], a1 = Ps[k][wm * 64 + 32 + l31];
    const float b0 = Rs[k][wn * 64 + l31], b1 = Rs[k][wn * 64 + 32 + l31];
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
  }
  // accumulator register r of a 32 x 32 tile is row (r & 3) + 8 (r >> 2) + 4 half, column lane & 31
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int gi = gi_base + mi * 32 + (r & 3) + 8 * (r >> 2);
      if (gi >= n) continue;
      const unsigned int pi = (unsigned int)(gi - k0);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int gj = gj_base + ni * 32;
        if (gj >= n) continue;
        const unsigned int pj = (unsigned int)(gj - k0);
        float v;
        if (pi < (unsigned int)SPD_B) v = Rs[pi][gj - j0];
        else if (pj < (unsigned int)SPD_B) v = R[(long)pj * ldp + gi];
        else v = cv[mi][ni][r] - acc[mi][ni][r];
        A[(long)gi * ld + gj] = sgn * v;
      }
    }
}

extern "C" long sbr_spd_inverse_f32_workspace(int n) {
  if (n <= 0) return 0;
  return (long)sizeof(float) * (SPD_B * SPD_B + 2L * SPD_B * spd_ldp(n));
}

extern "C" int sbr_spd_inverse_f32(float* A, int n, long ld, void* workspace, long workspace_bytes, int* info, void* stream) {
  SBR_REQUIRE(n >= 0 && n <= SPD_N_MAX, "%s: n=%d outside [0, 2^20]", __func__, n);
  if (n == 0) return SBR_OK;
  SBR_TRY(sbr_check_ld(__func__, "n", n, {{"ld", ld}}));
  SBR_REQUIRE_OPERANDS(__func__, A && info);
  SBR_REQUIRE_WORKSPACE(__func__, workspace, workspace_bytes, sbr_spd_inverse_f32_workspace(n), 16);
  hipStream_t s = (hipStream_t)stream;
  const long ldp = spd_ldp(n);
  float* Dinv = (float*)workspace;
  float* P = Dinv + SPD_B * SPD_B;
  float* R = P + SPD_B * ldp;
  const unsigned tiles = (unsigned)(ldp / SPD_T);
  for (int k0 = 0; k0 < n; k0 += SPD_B) {
    const int b = n - k0 < SPD_B ? n - k0 : SPD_B;
    spd_diag_kernel<<<1, 256, 0, s>>>(A, ld, k0, b, Dinv, info);
    spd_panel_kernel<<<(unsigned)(ldp / SPD_B), 256, 0, s>>>(A, ld, n, k0, b, Dinv, P, R, ldp);
    spd_update_kernel<<<dim3(tiles, tiles), 256, 0, s>>>(A, ld, n, k0, P, R, ldp, k0 + SPD_B >= n ? -1.f : 1.f);
  }
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}

// ---- the weights --------------------------------------------------------------------------------------------------------------------
__global__ void ease_diag_kernel(const float* __restrict__ P, long ld, int n, float* __restrict__ diag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) diag[i] = P[(long)i * ld + i];
}

__global__ __launch_bounds__(256) void ease_weights_kernel(float* __restrict__ P, long ld, int n, const float* __restrict__ diag) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float d = -diag[j];
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    float* e = P + (long)i * ld + j;
    *e = i == j ? 0.f : *e / d;
  }
}

extern "C" int sbr_ease_weights_f32(float* P, int n, long ld, float* diag, void* stream) {
  SBR_REQUIRE(n >= 0 && n <= SPD_N_MAX, "%s: n=%d outside [0, 2^20]", __func__, n);
  if (n == 0) return SBR_OK;
  SBR_TRY(sbr_check_ld(__func__, "n", n, {{"ld", ld}}));
  SBR_REQUIRE_OPERANDS(__func__, P && diag);
  ease_diag_kernel<<<sbr_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(P, ld, n, diag);
  ease_weights_kernel<<<dim3(sbr_cdiv(n, 256), n < 4096 ? n : 4096), 256, 0, (hipStream_t)stream>>>(P, ld, n, diag);
  SBR_CHECK_LAUNCH(__func__);
  return SBR_OK;
}
