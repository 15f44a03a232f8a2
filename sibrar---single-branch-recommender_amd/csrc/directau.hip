// The two loss terms of DirectAU (Wang et al., KDD 2022) for a batch of embedding rows, on the 64 x 64 fp32 tile skeleton (tile64_f32.h):
//   sbr_uniformity_fwd   S = sum_{i<j} w_ij,  loss = log(S * 2 / (n (n - 1))),  w_ij = exp(-t d_ij^2),  d_ij^2 = max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j)
//   sbr_uniformity_bwd   dx_i = g * (-2 t / S) * (x_i sum_{j != i} w_ij - sum_{j != i} w_ij x_j), w recomputed
//   sbr_align_fwd/_bwd   scale * sum_{label = 1} (2 - 2 z) over a logit matrix and its gradient (the alignment term on cosine logits)
// Nothing of size n x n reaches memory. A workgroup of 256 threads owns a tile of 64 rows, which it keeps transposed in LDS for its
// whole life ([D rounded up to 32][64 + 4] floats), and streams the column tiles past it in ascending order: a column tile is staged the
// same way, the 64 x 64 Gram tile is one fmaf chain per element over d = 0 .. D - 1 (t64_mma, a thread holds 4 x 4), and the squared norms
// come out of the staging (32 fmaf chains per row over d = sk, sk + 32, .., added by t64_half_sum<true>): the same function of the row
// whether it is staged as a row-tile or a column-tile row. The forward pass takes the column tiles from the row tile's own upwards and
// the pairs i < j of them; the backward pass takes every column tile and the pairs i != j, and multiplies the weight tile into the
// column tile's rows (read a second time, as stored) for the [64, D] accumulator that a thread keeps in registers (4 x 4 per 64 columns
// of D: the reason for D <= 256).
// Orders. Forward: a thread adds its 16 weights of a tile pair as ((w0 + w1) + (w2 + w3)) per row and ((r0 + r1) + (r2 + r3)) over its
// rows in fp32, and adds that to a double it keeps over the column tiles; the 256 doubles are added by sbr_wave_sum_d and then
// ((w0 + w1) + (w2 + w3)) over the waves into the row tile's partial; a second launch of one thread adds the partials in tile order and
// rounds to fp32 once. Backward: per row, the 4 weights a thread holds as above, the 16 threads of the row by t64_row_sum, the column
// tiles in ascending order, in fp32; per (row, d), one fmaf chain over j = 0 .. n - 1 (zero weights where the pair is excluded).
// Every output element has one owner and none of the orders depends on the grid: no atomics, the same bits for every max_wg.
// include/sibrar_hip.h states the definitions; tests/directau_ref.py derives the error bound from the geometry above.
#include "tile64_f32.h"
#include "det.h"

#define UNI_MAX_D 256
#define UNI_THREADS 256

// the whole tile j0 .. j0 + 63 of x [n, D], transposed: Xs[d][row] for d < 32 * chunks (zero past D and past n), sq[row] = |x_row|^2
__device__ __forceinline__ void uni_stage_tile(float* __restrict__ Xs, float* __restrict__ sq, const float* __restrict__ x, long j0, long n,
                                               int D, int t) {
  const int sk = t & 31, sr = t >> 5;
  const float* rp[8];
  t64_row_ptrs(rp, x, D, nullptr, j0, n, sr);
  float ss[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) ss[q] = 0.f;
  for (int d0 = 0; d0 < D; d0 += T64_KC) t64_stage_rows_t(Xs + d0 * T64_LD, rp, d0 + sk, D, sk, sr, ss, true);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float v = t64_half_sum<true>(ss[q]);
    if (sk == 0) sq[sr + 8 * q] = v;
  }
}

// w[i][c] = expf(-t max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j)) for row 4 rg + i of the row tile and column 4 cg + c of the column tile, and
// +0 where the pair is excluded: past n, the diagonal, and (UPPER) every pair with i >= j
template <bool UPPER>
__device__ __forceinline__ void uni_weights(const float* __restrict__ As, const float* __restrict__ Bs, const float* __restrict__ sqa,
                                            const float* __restrict__ sqb, long i0, long j0, long n, int D, float t_, int rg, int cg,
                                            float (&w)[4][4]) {
#pragma clang fp contract(off)
  t64_zero(w);
  for (int d0 = 0; d0 < D; d0 += T64_KC) t64_mma(As + d0 * T64_LD, Bs + d0 * T64_LD, rg, cg, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long gi = i0 + 4 * rg + i;
    const float a = sqa[4 * rg + i];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long gj = j0 + 4 * cg + c;
      const bool take = gi < n && gj < n && (UPPER ? gi < gj : gi != gj);
      const float d2 = fmaxf(0.f, (a + sqb[4 * cg + c]) - 2.f * w[i][c]);
      w[i][c] = take ? expf(-(t_ * d2)) : 0.f;
    }
  }
}

// ((w0 + w1) + (w2 + w3)) of a row of the thread's block
__device__ __forceinline__ float uni_row4(const float (&w)[4][4], int i) {
#pragma clang fp contract(off)
  return (w[i][0] + w[i][1]) + (w[i][2] + w[i][3]);
}

__global__ __launch_bounds__(UNI_THREADS) void uni_fwd_kernel(const float* __restrict__ x, long n, int D, float t_, double* __restrict__ part) {
  extern __shared__ __align__(16) float uni_lds[];
  __shared__ float sqa[T64_T], sqb[T64_T];
  __shared__ double red[UNI_THREADS / 64];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int Dp = (D + T64_KC - 1) / T64_KC * T64_KC, tiles = (int)((n + T64_T - 1) / T64_T);
  float* As = uni_lds;
  float* Bs = uni_lds + Dp * T64_LD;
  for (int rt = blockIdx.x; rt < tiles; rt += gridDim.x) {
    const long i0 = (long)rt * T64_T;
    uni_stage_tile(As, sqa, x, i0, n, D, t);
    double acc = 0.0;
    for (int ct = rt; ct < tiles; ++ct) {
      const long j0 = (long)ct * T64_T;
      uni_stage_tile(Bs, sqb, x, j0, n, D, t);
      __syncthreads();
      float w[4][4];
      uni_weights<true>(As, Bs, sqa, sqb, i0, j0, n, D, t_, rg, cg, w);
      acc += (double)((uni_row4(w, 0) + uni_row4(w, 1)) + (uni_row4(w, 2) + uni_row4(w, 3)));
      __syncthreads();                                             // Bs and sqb are free for the next column tile
    }
    acc = sbr_wave_sum_d(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) part[rt] = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();                                               // As, sqa and red are free for the next row tile
  }
}

// S = the partials in tile order, in double, rounded once; loss = log(S * 2 / (n (n - 1))) of that fp32 S, in double, rounded once
__global__ void uni_fold_kernel(const double* __restrict__ part, int tiles, long n, float* __restrict__ S, float* __restrict__ loss) {
  double s = 0.0;
  for (int i = 0; i < tiles; ++i) s += part[i];
  const float sf = (float)s;
  S[0] = sf;
  loss[0] = (float)log((double)sf * 2.0 / ((double)n * (double)(n - 1)));
}

template <int DT>   // 64-wide blocks of D a thread accumulates: tiles(D)
__global__ __launch_bounds__(UNI_THREADS) void uni_bwd_kernel(const float* __restrict__ x, long n, int D, float t_, const float* __restrict__ S,
                                                              const float* __restrict__ grad, float* __restrict__ dx) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float uni_lds[];
  __shared__ float sqa[T64_T], sqb[T64_T];
  __shared__ __align__(16) float Ps[T64_KC * T64_LD], Xs[T64_KC * T64_LD];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4, bc = t & 63, bk = t >> 6;
  const int Dp = (D + T64_KC - 1) / T64_KC * T64_KC, tiles = (int)((n + T64_T - 1) / T64_T);
  float* As = uni_lds;
  float* Bs = uni_lds + Dp * T64_LD;
  const float coef = grad[0] * (-2.f * t_ / S[0]);
  for (int rt = blockIdx.x; rt < tiles; rt += gridDim.x) {
    const long i0 = (long)rt * T64_T;
    uni_stage_tile(As, sqa, x, i0, n, D, t);
    float acc[DT][4][4], rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) t64_zero(acc[dt]);
    for (int ct = 0; ct < tiles; ++ct) {
      const long j0 = (long)ct * T64_T;
      uni_stage_tile(Bs, sqb, x, j0, n, D, t);
      __syncthreads();
      float w[4][4];
      uni_weights<false>(As, Bs, sqa, sqb, i0, j0, n, D, t_, rg, cg, w);
#pragma unroll
      for (int i = 0; i < 4; ++i) rs[i] = rs[i] + t64_row_sum(uni_row4(w, i));
      // acc[row, d] += sum_j w[row, j] x[j, d]: the weights transposed into Ps by halves of 32 columns, the rows j as stored into Xs
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const long n0 = j0 + half * T64_KC;
        if (n0 >= n) break;                                        // the same for every thread
        t64_stage_regs_t(Ps, w, half, rg, cg);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int k = bk + 4 * q, d = dt * T64_T + bc;
            const long j = n0 + k;
            Xs[k * T64_LD + bc] = (j < n && d < D) ? x[j * D + d] : 0.f;
          }
          __syncthreads();
          t64_mma(Ps, Xs, rg, cg, acc[dt]);
          __syncthreads();
        }
      }
      __syncthreads();                                             // Bs and sqb are free for the next column tile
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long gi = i0 + 4 * rg + i;
        if (gi >= n) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int d = dt * T64_T + 4 * cg + c;
          if (d < D) dx[gi * D + d] = coef * (x[gi * D + d] * rs[i] - acc[dt][i][c]);
        }
      }
    }
    __syncthreads();                                               // As and sqa are free for the next row tile
  }
}

static inline size_t uni_lds_bytes(int D) { return 2 * (size_t)((D + T64_KC - 1) / T64_KC * T64_KC) * T64_LD * sizeof(float); }

static int uni_check(const char* who, long n, int D, float t, int max_wg) {
  SBR_REQUIRE(n >= 2 && n <= INT_MAX, "%s: n=%ld rows, outside [2, 2^31): the term is a mean over pairs", who, n);
  SBR_REQUIRE(D >= 1 && D <= UNI_MAX_D, "%s: D=%d outside [1, %d]", who, D, UNI_MAX_D);
  SBR_REQUIRE(sbr_pos_finite(t), "%s: t=%g is not positive and finite", who, (double)t);
  SBR_REQUIRE(max_wg >= 0, "%s: negative max_wg %d", who, max_wg);
  return SBR_OK;
}

extern "C" long sbr_uniformity_workspace(long n, int D) {
  (void)D;
  return (long)sizeof(double) * (n > 0 ? (n + T64_T - 1) / T64_T : 1);
}

extern "C" int sbr_uniformity_fwd(const float* x, long n, int D, float t, float* S, float* loss, void* ws, long ws_bytes, int max_wg,
                                  void* stream) {
  if (int rc = uni_check("sbr_uniformity_fwd", n, D, t, max_wg)) return rc;
  SBR_REQUIRE(x && S && loss, "sbr_uniformity_fwd: null operand (x, S or loss)");
  SBR_REQUIRE(ws && ws_bytes >= sbr_uniformity_workspace(n, D), "sbr_uniformity_fwd: workspace too small");
  static SbrLdsSlot slot;
  const size_t lds = uni_lds_bytes(D);
  if (int rc = sbr_raise_lds("sbr_uniformity_fwd", (const void*)uni_fwd_kernel, &slot, lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = t64_tiles(n);
  uni_fwd_kernel<<<t64_wgs(n, max_wg > 0 ? max_wg : T64_MAX_WG), UNI_THREADS, lds, st>>>(x, n, D, t, (double*)ws);
  uni_fold_kernel<<<1, 1, 0, st>>>((const double*)ws, tiles, n, S, loss);
  SBR_CHECK_LAUNCH("sbr_uniformity_fwd");
  return SBR_OK;
}

extern "C" int sbr_uniformity_bwd(const float* x, long n, int D, float t, const float* S, const float* grad, float* dx, int max_wg,
                                  void* stream) {
  if (int rc = uni_check("sbr_uniformity_bwd", n, D, t, max_wg)) return rc;
  SBR_REQUIRE(x && S && grad && dx, "sbr_uniformity_bwd: null operand (x, S, grad or dx)");
  SBR_REQUIRE(!sbr_overlap(x, 4L * n * D, dx, 4L * n * D), "sbr_uniformity_bwd: dx overlaps x (rows are read while other rows are written)");
  const size_t lds = uni_lds_bytes(D);
  hipStream_t st = (hipStream_t)stream;
  const int wgs = t64_wgs(n, max_wg > 0 ? max_wg : T64_MAX_WG);
  int rc = SBR_OK;
  t64_dispatch_npt(t64_tiles(D), [&](auto dt) {
    static SbrLdsSlot slot;                                        // one per instantiation
    constexpr int DT = decltype(dt)::value;
    rc = sbr_raise_lds("sbr_uniformity_bwd", (const void*)uni_bwd_kernel<DT>, &slot, lds);
    if (rc == SBR_OK) uni_bwd_kernel<DT><<<wgs, UNI_THREADS, lds, st>>>(x, n, D, t, S, grad, dx);
  });
  if (rc) return rc;
  SBR_CHECK_LAUNCH("sbr_uniformity_bwd");
  return SBR_OK;
}

// ---- alignment: scale * sum over the positives of (2 - 2 z), one thread per logit row, block partials added in a fixed pattern ----------
#define ALIGN_THREADS 256

__global__ __launch_bounds__(ALIGN_THREADS) void align_fwd_kernel(const float* __restrict__ logits, const double* __restrict__ labels, long B,
                                                                  int N, double scale, double* __restrict__ part) {
  __shared__ double sm[ALIGN_THREADS / 64];
  const long b = blockIdx.x * (long)ALIGN_THREADS + threadIdx.x;
  double acc = 0.0;
  if (b < B)
    for (int j = 0; j < N; ++j)
      if (labels[b * N + j] == 1.0) acc += 2.0 - 2.0 * (double)logits[b * N + j];
  acc = sbr_wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (((sm[0] + sm[1]) + sm[2]) + sm[3]) * scale;
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_bwd_kernel(const double* __restrict__ labels, long BN, double scale,
                                                                  const void* __restrict__ gout, int gout_is_double,
                                                                  float* __restrict__ dlogits) {
  const long e = blockIdx.x * (long)ALIGN_THREADS + threadIdx.x;
  if (e >= BN) return;
  const double g = gout_is_double ? ((const double*)gout)[0] : (double)((const float*)gout)[0];
  dlogits[e] = labels[e] == 1.0 ? (float)(-2.0 * scale * g) : 0.f;
}

static __global__ void align_zero_kernel(double* __restrict__ p) { p[0] = 0.0; }

extern "C" int sbr_align_fwd(const float* logits, const double* labels, long B, int N, double scale, double* loss_out, void* stream) {
  SBR_REQUIRE(logits && labels && loss_out, "sbr_align_fwd: null operand");
  SBR_REQUIRE(B >= 0 && N >= 1, "sbr_align_fwd: B=%ld, N=%d: a negative batch or no columns", B, N);
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    align_zero_kernel<<<1, 1, 0, s>>>(loss_out);
    SBR_CHECK_LAUNCH("sbr_align_fwd");
    return SBR_OK;
  }
  const int nb = sbr_cdiv(B, ALIGN_THREADS);
  double* part = (double*)sbr_det_scratch(SBR_SCRATCH_LOSS, (size_t)nb * sizeof(double), s, "sbr_align_fwd");
  if (!part) return SBR_ERR_HIP;
  align_fwd_kernel<<<nb, ALIGN_THREADS, 0, s>>>(logits, labels, B, N, scale, part);
  return sbr_det_sum_partials(part, nb, loss_out, s, "sbr_align_fwd");
}

extern "C" int sbr_align_bwd(const double* labels, long B, int N, double scale, const void* grad_out, int grad_out_is_double, float* dlogits,
                             void* stream) {
  SBR_REQUIRE(labels && grad_out && dlogits, "sbr_align_bwd: null operand");
  SBR_REQUIRE(B >= 0 && N >= 1, "sbr_align_bwd: B=%ld, N=%d: a negative batch or no columns", B, N);
  if (B == 0) return SBR_OK;
  const long BN = B * (long)N;
  align_bwd_kernel<<<sbr_cdiv(BN, ALIGN_THREADS), ALIGN_THREADS, 0, (hipStream_t)stream>>>(labels, BN, scale, grad_out, grad_out_is_double,
                                                                                             dlogits);
  SBR_CHECK_LAUNCH("sbr_align_bwd");
  return SBR_OK;
}
