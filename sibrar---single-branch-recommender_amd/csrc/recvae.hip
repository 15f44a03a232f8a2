// The two row-wise tails of RecVAE (Shenbin et al., WSDM 2020): the encoder's layer tail and the composite-prior KL term. Four kernels
// behind five entries (include/sibrar_hip.h states the definitions and the order of every operation):
//   sbr_swish_ln_fwd / sbr_swish_ln_bwd   s = a + R_in, h = LayerNorm(swish(s)), R_out = R_in + h, and the backward pass with the column
//                                         sums d gamma, d beta (sbr_swish_ln_slabs: how many slabs of partials the backward pass writes)
//   sbr_prior_kl_fwd / sbr_prior_kl_bwd   z = mu + eps exp(logvar / 2) and row_kl = weight * sum_j (log q - log p) against the three-
//                                         component prior, and the gradients to mu and logvar
// One wave per row, the row in registers: element j of a row belongs to lane j % 64, which walks its elements in ascending order; a
// sum over the row is the lanes' partial sums added by an xor butterfly with the offsets 32, 16, .. 1. A workgroup holds RV_WAVES rows.
// Nothing depends on B, on the row's place in the batch or on the run, and there is no atomic anywhere: d gamma and d beta are slab
// partials in a caller's buffer, added in slab order by a second launch. No fma contraction: tests/recvae_ref.py restates the order.
#include "common.h"

#define RV_THREADS 256
#define RV_WAVES (RV_THREADS / 64)
#define RV_MAX_W 1024                  // the widest row: 16 elements per lane
#define RV_MAX_SLABS 1024              // slabs of the backward pass's column partials (and its workgroups)
#define RV_GRID_MAX (1 << 20)          // workgroups of the other launches; rows beyond are taken by a grid-stride loop

#define RV_LOG2PI 1.8378770664093453f
#define RV_LOGW0 -1.8971199848858813f  // log(3 / 20)
#define RV_LOGW1 -0.2876820724517809f  // log(3 / 4)
#define RV_LOGW2 -2.3025850929940457f  // log(1 / 10)
#define RV_V2 10.f                     // the wide component's log-variance
#define RV_EXP_V2 22026.465794806718f  // exp(10)

__device__ __forceinline__ float rv_sigmoid(float s) { return 1.f / (1.f + expf(-s)); }

// the float32 exponential, correctly rounded (through the double one): z has the same bits as a host restatement that does the same
__device__ __forceinline__ float rv_exp_cr(float x) { return (float)exp((double)x); }

// ---- swish + LayerNorm ----------------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(RV_THREADS) void rv_swish_ln_fwd_kernel(const float* __restrict__ a, const float* __restrict__ rin,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                     long B, int H, float* __restrict__ s_out, float* __restrict__ h,
                                                                     float* __restrict__ rout, float* __restrict__ mean, float* __restrict__ rstd) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const float fh = (float)H;
  for (long b = (long)blockIdx.x * RV_WAVES + (threadIdx.x >> 6); b < B; b += (long)gridDim.x * RV_WAVES) {
    const long base = b * H;
    float y[K], r[K];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      y[k] = 0.f;
      r[k] = 0.f;
      if (j < H) {
        float s = a[base + j];
        if (rin) {
          r[k] = rin[base + j];
          s = s + r[k];
        }
        s_out[base + j] = s;
        y[k] = s * rv_sigmoid(s);
        sum = sum + y[k];
      }
    }
    const float m = sbr_wave_sum(sum) / fh;
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (lane + 64 * k < H) {
        y[k] = y[k] - m;
        ss = ss + y[k] * y[k];
      }
    }
    const float rs = 1.f / sqrtf(sbr_wave_sum(ss) / fh + eps);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      if (j < H) {
        const float hv = y[k] * rs * gamma[j] + beta[j];
        h[base + j] = hv;
        if (rout) rout[base + j] = rin ? r[k] + hv : hv;
      }
    }
    if (lane == 0) {
      mean[b] = m;
      rstd[b] = rs;
    }
  }
}

// Workgroup w is slab w: the rows [w * RV_WAVES * rps, (w + 1) * RV_WAVES * rps), wave q taking the rows first + q, first + q +
// RV_WAVES, ... of them in that order. part (may be NULL): [slabs][2][H], the slab's sums of g * xhat and of g, a lane's rows in
// ascending order, then the waves in ascending order.
template <int K>
__global__ __launch_bounds__(RV_THREADS) void rv_swish_ln_bwd_kernel(const float* __restrict__ s_in, const float* __restrict__ mean,
                                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                     const float* __restrict__ dh, const float* __restrict__ dro, long B, int H,
                                                                     int rps, float* __restrict__ da, float* __restrict__ drin,
                                                                     float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float red[RV_WAVES][2][64 * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float fh = (float)H;
  const long first = (long)blockIdx.x * RV_WAVES * rps;
  float pg[K], pb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) pg[k] = pb[k] = 0.f;
  for (int i = 0; i < rps; ++i) {
    const long b = first + wave + (long)i * RV_WAVES;
    if (b >= B) break;
    const long base = b * H;
    const float m = mean[b], rs = rstd[b];
    float xh[K], gg[K], dsw[K];
    float sum1 = 0.f, sum2 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      xh[k] = gg[k] = dsw[k] = 0.f;
      if (j < H) {
        const float s = s_in[base + j];
        const float sig = rv_sigmoid(s);
        const float y = s * sig;
        xh[k] = (y - m) * rs;
        dsw[k] = sig + y * (1.f - sig);
        const float g = dh ? (dro ? dh[base + j] + dro[base + j] : dh[base + j]) : dro[base + j];
        gg[k] = g * gamma[j];
        sum1 = sum1 + gg[k];
        sum2 = sum2 + gg[k] * xh[k];
        pg[k] = pg[k] + g * xh[k];
        pb[k] = pb[k] + g;
      }
    }
    const float c1 = sbr_wave_sum(sum1) / fh, c2 = sbr_wave_sum(sum2) / fh;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      if (j < H) {
        const float ds = rs * ((gg[k] - c1) - xh[k] * c2) * dsw[k];
        da[base + j] = ds;
        if (drin) drin[base + j] = dro ? ds + dro[base + j] : ds;
      }
    }
  }
  if (!part) return;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    red[wave][0][lane + 64 * k] = pg[k];
    red[wave][1][lane + 64 * k] = pb[k];
  }
  __syncthreads();
  for (int j = threadIdx.x; j < H; j += RV_THREADS) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float t = red[0][q][j];
#pragma unroll
      for (int w = 1; w < RV_WAVES; ++w) t = t + red[w][q][j];
      part[((long)blockIdx.x * 2 + q) * H + j] = t;
    }
  }
}

// out[q][j] = the slabs' partials of column j added in slab order, in double, rounded once; q = 0: d gamma, 1: d beta
__global__ void rv_slab_sum_kernel(const float* __restrict__ part, int slabs, int H, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * H) return;
  const int q = i / H, j = i - q * H;
  double t = 0.0;
  for (int sl = 0; sl < slabs; ++sl) t += (double)part[((long)sl * 2 + q) * H + j];
  (q ? dbeta : dgamma)[j] = (float)t;
}

// ---- the composite prior ---------------------------------------------------------------------------------------------------------------
struct RvMix { float l0, l1, l2, mx, e0, e1, e2, se; };

// the three weighted log-densities of z, their maximum, and the exponentials relative to it
__device__ __forceinline__ RvMix rv_mix(float z, float mo, float lvo) {
#pragma clang fp contract(off)
  RvMix x;
  const float d = z - mo;
  x.l0 = RV_LOGW0 - 0.5f * (RV_LOG2PI + z * z);
  x.l1 = RV_LOGW1 - 0.5f * (lvo + RV_LOG2PI + d * d / expf(lvo));
  x.l2 = RV_LOGW2 - 0.5f * (RV_V2 + RV_LOG2PI + z * z / RV_EXP_V2);
  x.mx = fmaxf(fmaxf(x.l0, x.l1), x.l2);
  x.e0 = expf(x.l0 - x.mx);
  x.e1 = expf(x.l1 - x.mx);
  x.e2 = expf(x.l2 - x.mx);
  x.se = x.e0 + x.e1 + x.e2;
  return x;
}

template <int K>
__global__ __launch_bounds__(RV_THREADS) void rv_prior_kl_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                                     const float* __restrict__ eps, const float* __restrict__ mu_old,
                                                                     const float* __restrict__ logvar_old, const float* __restrict__ weight,
                                                                     long B, int L, float* __restrict__ z_out, float* __restrict__ row_kl) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  for (long b = (long)blockIdx.x * RV_WAVES + (threadIdx.x >> 6); b < B; b += (long)gridDim.x * RV_WAVES) {
    const long base = b * L;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      if (j < L) {
        const float lv = logvar[base + j], e = eps[base + j];
        const float z = mu[base + j] + e * rv_exp_cr(0.5f * lv);
        z_out[base + j] = z;
        const float lq = -0.5f * (lv + RV_LOG2PI + e * e);            // (z - mu)^2 / exp(logvar) is eps^2
        const RvMix x = rv_mix(z, mu_old[base + j], logvar_old[base + j]);
        acc = acc + (lq - (x.mx + logf(x.se)));
      }
    }
    acc = sbr_wave_sum(acc);
    if (lane == 0) row_kl[b] = weight[b] * acc;
  }
}

template <int K>
__global__ __launch_bounds__(RV_THREADS) void rv_prior_kl_bwd_kernel(const float* __restrict__ logvar, const float* __restrict__ eps,
                                                                     const float* __restrict__ mu_old, const float* __restrict__ logvar_old,
                                                                     const float* __restrict__ weight, const float* __restrict__ z_in,
                                                                     const float* __restrict__ dz, const float* __restrict__ gup, float scale,
                                                                     long B, int L, float* __restrict__ dmu, float* __restrict__ dlogvar) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const float up = gup ? gup[0] * scale : scale;
  for (long b = (long)blockIdx.x * RV_WAVES + (threadIdx.x >> 6); b < B; b += (long)gridDim.x * RV_WAVES) {
    const long base = b * L;
    const float c = up * weight[b];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      if (j < L) {
        const float z = z_in[base + j], mo = mu_old[base + j], lvo = logvar_old[base + j];
        const RvMix x = rv_mix(z, mo, lvo);
        // d log p / dz = sum_c p_c * (-(z - m_c) / exp(v_c)), p_c = e_c / se
        const float dlp = -((x.e0 * z + x.e1 * ((z - mo) / expf(lvo)) + x.e2 * (z / RV_EXP_V2)) / x.se);
        float t = -(c * dlp);
        if (dz) t = dz[base + j] + t;
        dmu[base + j] = t;
        dlogvar[base + j] = t * (0.5f * (eps[base + j] * rv_exp_cr(0.5f * logvar[base + j]))) - 0.5f * c;
      }
    }
  }
}

// ---- entries ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned rv_row_grid(long B) {
  const long blocks = (B + RV_WAVES - 1) / RV_WAVES;
  return (unsigned)(blocks < RV_GRID_MAX ? blocks : RV_GRID_MAX);
}

// rows of a slab's wave: the fewest that keep the slabs at RV_MAX_SLABS or below
static inline long rv_rows_per_wave(long B) {
  const long per = (long)RV_WAVES * RV_MAX_SLABS;
  return B <= per ? 1 : (B + per - 1) / per;
}

// the smallest instantiated K (elements per lane) that holds a row of `width`
#define RV_DISPATCH(width, KERNEL, grid, st, ...)                                                       \
  do {                                                                                                  \
    const int k__ = ((width) + 63) / 64;                                                                \
    if (k__ <= 1) KERNEL<1><<<grid, RV_THREADS, 0, st>>>(__VA_ARGS__);                                  \
    else if (k__ <= 2) KERNEL<2><<<grid, RV_THREADS, 0, st>>>(__VA_ARGS__);                             \
    else if (k__ <= 4) KERNEL<4><<<grid, RV_THREADS, 0, st>>>(__VA_ARGS__);                             \
    else if (k__ <= 8) KERNEL<8><<<grid, RV_THREADS, 0, st>>>(__VA_ARGS__);                             \
    else if (k__ <= 12) KERNEL<12><<<grid, RV_THREADS, 0, st>>>(__VA_ARGS__);                           \
    else KERNEL<16><<<grid, RV_THREADS, 0, st>>>(__VA_ARGS__);                                          \
  } while (0)

extern "C" int sbr_swish_ln_slabs(long B) {
  if (B <= 0) return 0;
  const long rows = RV_WAVES * rv_rows_per_wave(B);
  return (int)((B + rows - 1) / rows);
}

extern "C" int sbr_swish_ln_fwd(const float* a, const float* r_in, const float* gamma, const float* beta, float eps, long B, int H, float* s,
                                float* h, float* r_out, float* mean, float* rstd, void* stream) {
  SBR_REQUIRE(H >= 1 && H <= RV_MAX_W, "sbr_swish_ln_fwd: H=%d outside [1, %d]", H, RV_MAX_W);
  SBR_REQUIRE(B >= 0, "sbr_swish_ln_fwd: B=%ld is negative", B);
  SBR_REQUIRE(sbr_pos_finite(eps), "sbr_swish_ln_fwd: eps=%g is not positive and finite", (double)eps);
  SBR_REQUIRE(a && gamma && beta && s && h && mean && rstd, "sbr_swish_ln_fwd: null operand (a, gamma, beta, s, h, mean or rstd)");
  if (B == 0) return SBR_OK;
  hipStream_t st = (hipStream_t)stream;
  RV_DISPATCH(H, rv_swish_ln_fwd_kernel, rv_row_grid(B), st, a, r_in, gamma, beta, eps, B, H, s, h, r_out, mean, rstd);
  SBR_CHECK_LAUNCH("sbr_swish_ln_fwd");
  return SBR_OK;
}

extern "C" int sbr_swish_ln_bwd(const float* s, const float* mean, const float* rstd, const float* gamma, const float* dh, const float* dr_out,
                                long B, int H, float* da, float* dr_in, float* dgamma, float* dbeta, float* partials, void* stream) {
  SBR_REQUIRE(H >= 1 && H <= RV_MAX_W, "sbr_swish_ln_bwd: H=%d outside [1, %d]", H, RV_MAX_W);
  SBR_REQUIRE(B >= 0, "sbr_swish_ln_bwd: B=%ld is negative", B);
  SBR_REQUIRE(s && mean && rstd && gamma && da, "sbr_swish_ln_bwd: null operand (s, mean, rstd, gamma or da)");
  SBR_REQUIRE(dh || dr_out, "sbr_swish_ln_bwd: dh and dr_out are both null");
  SBR_REQUIRE((dgamma != nullptr) == (dbeta != nullptr) && (dgamma != nullptr) == (partials != nullptr),
              "sbr_swish_ln_bwd: dgamma, dbeta and partials are given together or not at all");
  if (B == 0) return SBR_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rps = (int)rv_rows_per_wave(B), slabs = sbr_swish_ln_slabs(B);
  RV_DISPATCH(H, rv_swish_ln_bwd_kernel, (unsigned)slabs, st, s, mean, rstd, gamma, dh, dr_out, B, H, rps, da, dr_in, partials);
  SBR_CHECK_LAUNCH("sbr_swish_ln_bwd");
  if (partials) {
    rv_slab_sum_kernel<<<(2 * H + 255) / 256, 256, 0, st>>>(partials, slabs, H, dgamma, dbeta);
    SBR_CHECK_LAUNCH("sbr_swish_ln_bwd");
  }
  return SBR_OK;
}

extern "C" int sbr_prior_kl_fwd(const float* mu, const float* logvar, const float* eps, const float* mu_old, const float* logvar_old,
                                const float* weight, long B, int L, float* z, float* row_kl, void* stream) {
  SBR_REQUIRE(L >= 1 && L <= RV_MAX_W, "sbr_prior_kl_fwd: L=%d outside [1, %d]", L, RV_MAX_W);
  SBR_REQUIRE(B >= 0, "sbr_prior_kl_fwd: B=%ld is negative", B);
  SBR_REQUIRE(mu && logvar && eps && mu_old && logvar_old && weight && z && row_kl,
              "sbr_prior_kl_fwd: null operand (mu, logvar, eps, mu_old, logvar_old, weight, z or row_kl)");
  if (B == 0) return SBR_OK;
  hipStream_t st = (hipStream_t)stream;
  RV_DISPATCH(L, rv_prior_kl_fwd_kernel, rv_row_grid(B), st, mu, logvar, eps, mu_old, logvar_old, weight, B, L, z, row_kl);
  SBR_CHECK_LAUNCH("sbr_prior_kl_fwd");
  return SBR_OK;
}

extern "C" int sbr_prior_kl_bwd(const float* logvar, const float* eps, const float* mu_old, const float* logvar_old, const float* weight,
                                const float* z, const float* dz, const float* upstream, float scale, long B, int L, float* dmu, float* dlogvar,
                                void* stream) {
  SBR_REQUIRE(L >= 1 && L <= RV_MAX_W, "sbr_prior_kl_bwd: L=%d outside [1, %d]", L, RV_MAX_W);
  SBR_REQUIRE(B >= 0, "sbr_prior_kl_bwd: B=%ld is negative", B);
  SBR_REQUIRE(logvar && eps && mu_old && logvar_old && weight && z && dmu && dlogvar,
              "sbr_prior_kl_bwd: null operand (logvar, eps, mu_old, logvar_old, weight, z, dmu or dlogvar)");
  if (B == 0) return SBR_OK;
  hipStream_t st = (hipStream_t)stream;
  RV_DISPATCH(L, rv_prior_kl_bwd_kernel, rv_row_grid(B), st, logvar, eps, mu_old, logvar_old, weight, z, dz, upstream, scale, B, L, dmu, dlogvar);
  SBR_CHECK_LAUNCH("sbr_prior_kl_bwd");
  return SBR_OK;
}
