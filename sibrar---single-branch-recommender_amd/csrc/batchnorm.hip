// BatchNorm1d over the row dimension of an [R, D] activation matrix, fused with the following activation
// (modules/polylinear.py:61-65, 68; algorithms/sgd_alg.py:1837). torch defaults: eps 1e-5, momentum 0.1, the running
// variance is the unbiased batch variance, normalisation uses the biased one.
//
// Train forward:  pass 1 column sums (sum x, sum x^2) in double -> ws[2*D] ; pass 2 normalise + affine + activation.
// Train backward: pass 1 column sums of dz and dz*xhat        -> ws[2*D] ; pass 2 dx = w*rstd*(dz - mean(dz) - xhat*mean(dz*xhat)).
// HBM-bound: forward reads X twice and writes Y once (12 B/element), backward reads X, Y, dY twice and writes dX.
#include "common.h"
#include "colred.h"

// generic fallback (colred.h: sbr_col_reduce_generic): sum x, sum x^2 in double
__global__ void bn_stats_kernel(const float* __restrict__ X, long n, int D, double* __restrict__ ws) {
  sbr_col_reduce_generic<2>(n, D, ws, [&](long j, int c, double* v) {
    const double x = (double)X[j * D + c];
    v[0] = x;
    v[1] = x * x;
  });
}

// The vector form (colred.h: geometry and publish tail), with the squares formed and both sums carried in DOUBLE from the first
// addition: the finaliser takes var = ss / n - m * m, whose cancellation multiplies every relative error of ss and of m by
// (mean / std)^2. With fp32 squares and fp32 per-thread sums the
// variance of a column with mean / std = 256 was off by 5e-4 (numerical contract of the BatchNorm statistics); with
// exact squares of fp32 values (24 + 24 bits fit a double) and double sums it is as good as the generic kernel's. The kernel
// stays bound by its one read of X.
__device__ __forceinline__ void bn_acc4(const float4 x, double* s, double* q) {
  const double a = (double)x.x, b = (double)x.y, c = (double)x.z, d = (double)x.w;
  s[0] += a; s[1] += b; s[2] += c; s[3] += d;
  q[0] = fma(a, a, q[0]); q[1] = fma(b, b, q[1]); q[2] = fma(c, c, q[2]); q[3] = fma(d, d, q[3]);
}

__global__ __launch_bounds__(256) void bn_stats4_kernel(const float* __restrict__ X, long n, int D, double* __restrict__ ws,
                                                        double* __restrict__ slots) {
  __shared__ double sm[2][4][256];
  const SbrColGeom g(n, D);
  const int RL = g.RL, t = threadIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  if (g.rl < RL) {
    const float* xp = X + 4 * g.cg;
    long j = g.lo + g.rl;
    for (; j + 3L * RL < g.hi; j += 4L * RL) {       // four independent 16-byte loads in flight
      const float4 x0 = *reinterpret_cast<const float4*>(xp + j * D), x1 = *reinterpret_cast<const float4*>(xp + (j + RL) * D),
                   x2 = *reinterpret_cast<const float4*>(xp + (j + 2L * RL) * D), x3 = *reinterpret_cast<const float4*>(xp + (j + 3L * RL) * D);
      bn_acc4(x0, s, q); bn_acc4(x1, s, q); bn_acc4(x2, s, q); bn_acc4(x3, s, q);
    }
    for (; j < g.hi; j += RL) bn_acc4(*reinterpret_cast<const float4*>(xp + j * D), s, q);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) { sm[0][i][t] = s[i]; sm[1][i][t] = q[i]; }
  __syncthreads();
  sbr_colred_publish(sm, g, D, ws, slots);
}

// one thread per column: batch mean / rstd, running-stat update
__global__ void bn_finalize_kernel(double* __restrict__ ws, long n, int D, float eps, float momentum,
                                   float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ running_mean,
                                   float* __restrict__ running_var, long* __restrict__ num_batches) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && num_batches) num_batches[0] += 1;
  if (c >= D) return;
  const double sum = sbr_colred_take(ws, 2 * D, c);                           // also re-zeroes the replicas
  const double sq = sbr_colred_take(ws, 2 * D, D + c);
  sbr_bn_finish_column(sum, sq, n, c, eps, momentum, mean, rstd, running_mean, running_var);
}

__global__ void bn_apply_kernel(const float* __restrict__ X, float* __restrict__ Y, long n, int D,
                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                const float* __restrict__ w, const float* __restrict__ b, int act) {
  const long total = n * D;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % D);
    Y[e] = sbr_act((X[e] - mean[c]) * rstd[c] * w[c] + b[c], act);
  }
}

// eval mode: running statistics
__global__ void bn_eval_kernel(const float* __restrict__ X, float* __restrict__ Y, long n, int D,
                               const float* __restrict__ rm, const float* __restrict__ rv, const float* __restrict__ w,
                               const float* __restrict__ b, float eps, int act) {
  const long total = n * D;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % D);
    Y[e] = sbr_act((X[e] - rm[c]) / sqrtf(rv[c] + eps) * w[c] + b[c], act);
  }
}

static int grid1d(long total) {
  int b = sbr_cdiv(total, 256);
  return b > 4096 ? 4096 : (b < 1 ? 1 : b);
}

// workspace ws: 34*D doubles (2*D totals + 16 replicas, see colred.h), ZERO on first use; every call
// leaves the replica part zeroed again (no memset per call)
static int bn_train_stats(const float* X, long n, int D, float* running_mean, float* running_var, long* num_batches_tracked,
                          float* save_mean, float* save_rstd, double* ws, float eps, float momentum, hipStream_t s) {
  const int rc = sbr_colred_dispatch(
      "sbr_bn_train_fwd/stats", 'D', n, D, 2, sbr_col_reduce_ok(X, D, D), ws, s,
      [&](int blocks, double* slots) { bn_stats4_kernel<<<blocks, 256, 0, s>>>(X, n, D, ws, slots); },
      [&](dim3 grid, double* rep1) { bn_stats_kernel<<<grid, 256, 0, s>>>(X, n, D, rep1); });
  if (rc) return rc;
  SBR_CHECK_LAUNCH("sbr_bn_train_fwd/stats");
  bn_finalize_kernel<<<sbr_cdiv(D, 256), 256, 0, s>>>(ws, n, D, eps, momentum, save_mean, save_rstd, running_mean,
                                                      running_var, num_batches_tracked);
  SBR_CHECK_LAUNCH("sbr_bn_train_fwd/finalize");
  return SBR_OK;
}

extern "C" int sbr_bn_train_fwd(const float* X, float* Y, long n, int D, const float* weight, const float* bias,
                                float* running_mean, float* running_var, long* num_batches_tracked, float* save_mean,
                                float* save_rstd, double* ws, float eps, float momentum, int act, void* stream) {
  SBR_REQUIRE(X && Y && weight && bias && save_mean && save_rstd && ws, "sbr_bn_train_fwd: null operand");
  SBR_REQUIRE(n >= 1, "sbr_bn_train_fwd: BatchNorm needs at least one row");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bn_train_stats(X, n, D, running_mean, running_var, num_batches_tracked, save_mean, save_rstd, ws, eps, momentum, s);
  if (rc != SBR_OK) return rc;
  bn_apply_kernel<<<grid1d(n * D), 256, 0, s>>>(X, Y, n, D, save_mean, save_rstd, weight, bias, act);
  SBR_CHECK_LAUNCH("sbr_bn_train_fwd/apply");
  return SBR_OK;
}

// statistics half of sbr_bn_train_fwd (batch mean / rstd, running-statistics update) without the normalising pass: the
// consumer applies the normalisation itself (fused_tail.hip: sbr_bn_score_fwd)
extern "C" int sbr_bn_train_stats(const float* X, long n, int D, float* running_mean, float* running_var,
                                  long* num_batches_tracked, float* save_mean, float* save_rstd, double* ws, float eps,
                                  float momentum, void* stream) {
  SBR_REQUIRE(X && save_mean && save_rstd && ws, "sbr_bn_train_stats: null operand");
  SBR_REQUIRE(n >= 1, "sbr_bn_train_stats: BatchNorm needs at least one row");
  return bn_train_stats(X, n, D, running_mean, running_var, num_batches_tracked, save_mean, save_rstd, ws, eps, momentum,
                        (hipStream_t)stream);
}

// second half of sbr_bn_train_stats for statistics that a producer kernel has already left pending in `ws` (the NT GEMM in front
// of the BatchNorm: sbr_gemm_split_f32 mode 0 with colsum_ws): batch mean / rstd of the n rows, running-statistics update
extern "C" int sbr_bn_finalize_stats(long n, int D, float* running_mean, float* running_var, long* num_batches_tracked,
                                     float* save_mean, float* save_rstd, double* ws, float eps, float momentum, void* stream) {
  SBR_REQUIRE(save_mean && save_rstd && ws && n >= 1 && D >= 1, "sbr_bn_finalize_stats: bad arguments");
  bn_finalize_kernel<<<sbr_cdiv(D, 256), 256, 0, (hipStream_t)stream>>>(ws, n, D, eps, momentum, save_mean, save_rstd, running_mean,
                                                                        running_var, num_batches_tracked);
  SBR_CHECK_LAUNCH("sbr_bn_finalize_stats");
  return SBR_OK;
}

extern "C" int sbr_bn_eval_fwd(const float* X, float* Y, long n, int D, const float* weight, const float* bias,
                               const float* running_mean, const float* running_var, float eps, int act, void* stream) {
  if (n == 0) return SBR_OK;
  SBR_REQUIRE(X && Y && weight && bias && running_mean && running_var, "sbr_bn_eval_fwd: null operand");
  bn_eval_kernel<<<grid1d(n * D), 256, 0, (hipStream_t)stream>>>(X, Y, n, D, running_mean, running_var, weight, bias, eps, act);
  SBR_CHECK_LAUNCH("sbr_bn_eval_fwd");
  return SBR_OK;
}

// ---- backward ------------------------------------------------------------------------------------------------------
// dz = dY * act'(Y);  ws[c] = sum dz ; ws[D + c] = sum dz * xhat
__global__ void bn_bwd_stats_kernel(const float* __restrict__ dY, const float* __restrict__ Y, const float* __restrict__ X,
                                    long n, int D, const float* __restrict__ mean, const float* __restrict__ rstd, int act,
                                    double* __restrict__ ws) {
  const int c0 = blockIdx.y * 64 + (threadIdx.x & 63);
  const float m = c0 < D ? mean[c0] : 0.f, r = c0 < D ? rstd[c0] : 0.f;
  sbr_col_reduce_generic<2>(n, D, ws, [&](long j, int c, double* v) {
    const long e = j * D + c;
    const float dz = dY[e] * sbr_act_grad_from_out(Y[e], act);
    v[0] = (double)dz;
    v[1] = (double)(dz * ((X[e] - m) * r));
  });
}

__global__ __launch_bounds__(256) void bn_bwd_stats4_kernel(const float* __restrict__ dY, const float* __restrict__ Y,
                                                            const float* __restrict__ X, long n, int D,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            int act, double* __restrict__ ws, double* __restrict__ slots) {
  const int cg0 = threadIdx.x % (D >> 2);
  const float4 m = *reinterpret_cast<const float4*>(mean + 4 * cg0), r = *reinterpret_cast<const float4*>(rstd + 4 * cg0);
  sbr_col_reduce<2>(n, D, ws, [&](long j, int cg, float4* v) {
    const long e = j * D + 4 * cg;
    const float4 g = *reinterpret_cast<const float4*>(dY + e), y = *reinterpret_cast<const float4*>(Y + e),
                 x = *reinterpret_cast<const float4*>(X + e);
    float4 dz;
    dz.x = g.x * sbr_act_grad_from_out(y.x, act); dz.y = g.y * sbr_act_grad_from_out(y.y, act);
    dz.z = g.z * sbr_act_grad_from_out(y.z, act); dz.w = g.w * sbr_act_grad_from_out(y.w, act);
    v[0] = dz;
    v[1] = make_float4(dz.x * ((x.x - m.x) * r.x), dz.y * ((x.y - m.y) * r.y), dz.z * ((x.z - m.z) * r.z),
                       dz.w * ((x.w - m.w) * r.w));
  }, slots);
}

__global__ void bn_bwd_apply_kernel(const float* __restrict__ dY, const float* __restrict__ Y, const float* __restrict__ X,
                                    float* __restrict__ dX, long n, int D, const float* __restrict__ mean,
                                    const float* __restrict__ rstd, const float* __restrict__ w, int act,
                                    const double* __restrict__ ws, float* __restrict__ dW, float* __restrict__ dB) {
  const long total = n * D;
  const double inv_n = 1.0 / (double)n;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % D);
    const float dz = dY[e] * sbr_act_grad_from_out(Y[e], act);
    const float xhat = (X[e] - mean[c]) * rstd[c];
    const float mdz = (float)(ws[c] * inv_n), mdzx = (float)(ws[D + c] * inv_n);
    dX[e] = w[c] * rstd[c] * (dz - mdz - xhat * mdzx);
    if (e < D) {       // first row's threads also publish the affine gradients
      dB[c] = (float)ws[c];
      dW[c] = (float)ws[D + c];
    }
  }
}

extern "C" int sbr_bn_train_bwd(const float* dY, const float* Y, const float* X, float* dX, long n, int D,
                                const float* weight, const float* save_mean, const float* save_rstd, float* dWeight,
                                float* dBias, double* ws, int act, void* stream) {
  SBR_REQUIRE(dY && Y && X && dX && weight && save_mean && save_rstd && dWeight && dBias && ws, "sbr_bn_train_bwd: null operand");
  SBR_REQUIRE(n >= 1, "sbr_bn_train_bwd: empty batch");
  hipStream_t s = (hipStream_t)stream;
  const bool vec_ok = sbr_col_reduce_ok(X, D, D) && ((((uintptr_t)dY) | ((uintptr_t)Y) | ((uintptr_t)save_mean) | ((uintptr_t)save_rstd)) & 15) == 0;
  const int rc = sbr_colred_dispatch(
      "sbr_bn_train_bwd", 'D', n, D, 2, vec_ok, ws, s,
      [&](int blocks, double* slots) { bn_bwd_stats4_kernel<<<blocks, 256, 0, s>>>(dY, Y, X, n, D, save_mean, save_rstd, act, ws, slots); },
      [&](dim3 grid, double* rep1) { bn_bwd_stats_kernel<<<grid, 256, 0, s>>>(dY, Y, X, n, D, save_mean, save_rstd, act, rep1); });
  if (rc) return rc;
  sbr_colred_final_kernel<<<sbr_cdiv(2 * D, 256), 256, 0, s>>>(ws, 2 * D);
  SBR_CHECK_LAUNCH("sbr_bn_train_bwd/stats");
  bn_bwd_apply_kernel<<<grid1d(n * D), 256, 0, s>>>(dY, Y, X, dX, n, D, save_mean, save_rstd, weight, act, ws, dWeight, dBias);
  SBR_CHECK_LAUNCH("sbr_bn_train_bwd/apply");
  return SBR_OK;
}
