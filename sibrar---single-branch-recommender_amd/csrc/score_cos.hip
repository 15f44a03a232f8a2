// DeepMF's scorer (algorithms/sgd_alg.py:1238-1242): nn.CosineSimilarity(dim=-1)(u[:, None, :], i) followed by the floor
// sim[sim < mu] = mu (equation 13 of Xue et al., IJCAI 2017), training form u [B, D] x i [B, N, D] -> [B, N], forward and backward,
// and the in-place floor of the all-pairs evaluation form.
//
// Arithmetic form. torch's cosine_similarity (2.x) clamps EACH norm at eps and normalises before it sums:
//     cos = sum_d (u_d / max(|u|, eps)) * (i_d / max(|i|, eps))
// (not dot / max(|u| |i|, eps): the two differ for rows shorter than eps; the G17 fixture, written by the real reference, pins the
// choice). Here the user row is divided by its clamped norm once, the products with the raw item row are summed, and the sum is
// divided by the item row's clamped norm: the same value with two roundings fewer per term.
// Its autograd treats the clamp as transparent for the norm's own gradient (the clamp is applied in place outside the tape), so with
// n = |x|, nc = max(n, eps):   d(x / nc) = I / nc - x x^T / (n nc), and the second term is zero for n = 0. Both factors are stored
// by the forward pass per row — 1 / nc and (n > 0 ? 1 / n : 0) — next to the un-floored cosine, and the backward pass derives no norm.
// A floored entry (cos < mu; a NaN is not below mu and stays) passes no gradient: the reference assigns by index, which cuts the tape.
//
// Work-item map: one wavefront per batch row b (four per workgroup). u[b] sits in registers for the whole row (up to 1024 columns;
// wider rows are re-read through the cache), the N item rows are streamed once — float4 per lane when D % 4 == 0 and every pointer
// is 16-byte aligned, one float per lane otherwise —, the dot product and the squared norms are reduced with wave shuffles, and in
// the backward pass the wave adds dU[b] up over n = 0 .. N-1 in registers in that order and writes every dI[b, n] itself. No LDS, no
// atomics: both kernels give the same bits on every run, in either mode of sbr_set_deterministic.
#include "common.h"

namespace {

// columns owned by a lane: chunk k covers [64 V k, 64 V (k + 1)), lane l its columns V l .. V l + V - 1
template <int V>
__device__ __forceinline__ void cos_load(const float* __restrict__ p, int c, int D, float (&v)[V]) {
  if constexpr (V == 4) {
    if (c < D) {
      const float4 q = *reinterpret_cast<const float4*>(p + c);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  } else {
    v[0] = c < D ? p[c] : 0.f;
  }
}

template <int V>
__device__ __forceinline__ void cos_store(float* __restrict__ p, int c, int D, const float (&v)[V]) {
  if (c >= D) return;
  if constexpr (V == 4) *reinterpret_cast<float4*>(p + c) = make_float4(v[0], v[1], v[2], v[3]);
  else p[c] = v[0];
}

// stats rows: [2] = {1 / max(|x|, eps), |x| > 0 ? 1 / |x| : 0}
__device__ __forceinline__ void cos_stats(float ss, float eps, float& nc, float& inv_c, float& inv_n) {
  const float n = sqrtf(ss);
  nc = fmaxf(n, eps);
  inv_c = 1.f / nc;
  inv_n = n > 0.f ? 1.f / n : 0.f;
}

template <int V, int NCH>
__global__ __launch_bounds__(256) void score_cos_fwd_kernel(const float* __restrict__ U, const float* __restrict__ I,
                                                            float* __restrict__ out, float* __restrict__ cos_raw,
                                                            float* __restrict__ u_stat, float* __restrict__ i_stat, long B, int N,
                                                            int D, float mu, float eps) {
  const long b = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  float u[NCH][V];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    cos_load<V>(U + b * D, (k * 64 + lane) * V, D, u[k]);
#pragma unroll
    for (int e = 0; e < V; ++e) ss += u[k][e] * u[k][e];
  }
  ss = sbr_wave_sum(ss);
  float nc, inv_c, inv_n;
  cos_stats(ss, eps, nc, inv_c, inv_n);
  if (lane == 0) { u_stat[2 * b] = inv_c; u_stat[2 * b + 1] = inv_n; }
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < V; ++e) u[k][e] = u[k][e] / nc;
  for (int n = 0; n < N; ++n) {
    const long s = b * N + n;
    const float* ip = I + s * D;
    float dot = 0.f, si = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      float v[V];
      cos_load<V>(ip, (k * 64 + lane) * V, D, v);
#pragma unroll
      for (int e = 0; e < V; ++e) { dot += u[k][e] * v[e]; si += v[e] * v[e]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { dot += __shfl_xor(dot, o, 64); si += __shfl_xor(si, o, 64); }
    float nci, iinv_c, iinv_n;
    cos_stats(si, eps, nci, iinv_c, iinv_n);
    const float c = dot / nci;
    if (lane == 0) {
      cos_raw[s] = c;
      out[s] = c < mu ? mu : c;
      i_stat[2 * s] = iinv_c;
      i_stat[2 * s + 1] = iinv_n;
    }
  }
}

// rows wider than the register form (D > 1024): the same sums, u[b] re-read through the cache
__global__ __launch_bounds__(256) void score_cos_fwd_wide_kernel(const float* __restrict__ U, const float* __restrict__ I,
                                                                 float* __restrict__ out, float* __restrict__ cos_raw,
                                                                 float* __restrict__ u_stat, float* __restrict__ i_stat, long B, int N,
                                                                 int D, float mu, float eps) {
  const long b = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const float* up = U + b * D;
  float ss = 0.f;
  for (int c = lane; c < D; c += 64) ss += up[c] * up[c];
  ss = sbr_wave_sum(ss);
  float nc, inv_c, inv_n;
  cos_stats(ss, eps, nc, inv_c, inv_n);
  if (lane == 0) { u_stat[2 * b] = inv_c; u_stat[2 * b + 1] = inv_n; }
  for (int n = 0; n < N; ++n) {
    const long s = b * N + n;
    const float* ip = I + s * D;
    float dot = 0.f, si = 0.f;
    for (int c = lane; c < D; c += 64) { const float v = ip[c]; dot += (up[c] / nc) * v; si += v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { dot += __shfl_xor(dot, o, 64); si += __shfl_xor(si, o, 64); }
    float nci, iinv_c, iinv_n;
    cos_stats(si, eps, nci, iinv_c, iinv_n);
    const float c = dot / nci;
    if (lane == 0) {
      cos_raw[s] = c;
      out[s] = c < mu ? mu : c;
      i_stat[2 * s] = iinv_c;
      i_stat[2 * s + 1] = iinv_n;
    }
  }
}

// per entry (b, n), with g' = 0 where the entry was floored:
//   a = g' / (nc_u nc_i)              dI[b, n] = a u - q i,   q = g' cos / (n_i nc_i)
//   dU[b] = sum_n a i[b, n]  -  u (sum_n g' cos) / (n_u nc_u)
struct CosCoef { float a, q, gc; };

__device__ __forceinline__ CosCoef cos_coef(const float* __restrict__ G, const float* __restrict__ cos_raw,
                                            const float* __restrict__ i_stat, long s, float mu, float u_inv_c) {
  const float c = cos_raw[s];
  const float g = c < mu ? 0.f : G[s];
  const float ic = i_stat[2 * s], in = i_stat[2 * s + 1];
  CosCoef k;
  k.a = g * u_inv_c * ic;
  k.q = g * ((c * in) * ic);          // |c| <= n_i / nc_i: c / n_i stays below 1 / nc_i, nothing overflows on the way
  k.gc = g * c;
  return k;
}

template <int V, int NCH>
__global__ __launch_bounds__(256) void score_cos_bwd_kernel(const float* __restrict__ G, const float* __restrict__ U,
                                                            const float* __restrict__ I, const float* __restrict__ cos_raw,
                                                            const float* __restrict__ u_stat, const float* __restrict__ i_stat,
                                                            float* __restrict__ dU, float* __restrict__ dI, long B, int N, int D,
                                                            float mu) {
  const long b = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  float u[NCH][V], acc[NCH][V];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    cos_load<V>(U + b * D, (k * 64 + lane) * V, D, u[k]);
#pragma unroll
    for (int e = 0; e < V; ++e) acc[k][e] = 0.f;
  }
  const float u_inv_c = u_stat[2 * b], u_inv_n = u_stat[2 * b + 1];
  float sgc = 0.f;
  for (int n = 0; n < N; ++n) {
    const long s = b * N + n;
    const CosCoef k_ = cos_coef(G, cos_raw, i_stat, s, mu, u_inv_c);
    sgc += k_.gc;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = (k * 64 + lane) * V;
      float v[V], d[V];
      cos_load<V>(I + s * D, c, D, v);
#pragma unroll
      for (int e = 0; e < V; ++e) { acc[k][e] += k_.a * v[e]; d[e] = k_.a * u[k][e] - k_.q * v[e]; }
      if (dI) cos_store<V>(dI + s * D, c, D, d);
    }
  }
  if (!dU) return;
  const float t = (u_inv_n * u_inv_c) * sgc;
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    float d[V];
#pragma unroll
    for (int e = 0; e < V; ++e) d[e] = acc[k][e] - u[k][e] * t;
    cos_store<V>(dU + b * D, (k * 64 + lane) * V, D, d);
  }
}

__global__ __launch_bounds__(256) void score_cos_bwd_wide_kernel(const float* __restrict__ G, const float* __restrict__ U,
                                                                 const float* __restrict__ I, const float* __restrict__ cos_raw,
                                                                 const float* __restrict__ u_stat, const float* __restrict__ i_stat,
                                                                 float* __restrict__ dU, float* __restrict__ dI, long B, int N, int D,
                                                                 float mu) {
  const long b = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const float u_inv_c = u_stat[2 * b], u_inv_n = u_stat[2 * b + 1];
  float sgc = 0.f;
  for (int n = 0; n < N; ++n) sgc += cos_coef(G, cos_raw, i_stat, b * N + n, mu, u_inv_c).gc;
  const float t = (u_inv_n * u_inv_c) * sgc;
  for (int c = lane; c < D; c += 64) {
    const float u = U[b * D + c];
    float acc = 0.f;
    for (int n = 0; n < N; ++n) {
      const long s = b * N + n;
      const CosCoef k_ = cos_coef(G, cos_raw, i_stat, s, mu, u_inv_c);
      const float v = I[s * D + c];
      acc += k_.a * v;
      if (dI) dI[s * D + c] = k_.a * u - k_.q * v;
    }
    if (dU) dU[b * D + c] = acc - u * t;
  }
}

// x[x < mu] = mu in place (a NaN is not below mu and stays)
__global__ void floor_scores_kernel(float* __restrict__ x, long n, long n_cols, long ld, float mu) {
  const long total = n * n_cols;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long r = e / n_cols;
    float* p = x + r * ld + (e - r * n_cols);
    const float v = *p;
    if (v < mu) *p = mu;
  }
}

inline bool cos_vec_ok(int D, const void* a, const void* b, const void* c, const void* d) {
  return (D & 3) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

}  // namespace

// V = 4: chunks of 256 columns; V = 1: chunks of 64 columns; both hold rows up to 1024 columns in registers
#define SBR_COS_DISPATCH(KERNEL, vec, D, ...)                                                       \
  do {                                                                                              \
    if (vec) {                                                                                      \
      if ((D) <= 256) KERNEL<4, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);                               \
      else if ((D) <= 512) KERNEL<4, 2><<<grid, 256, 0, s>>>(__VA_ARGS__);                          \
      else KERNEL<4, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);                                          \
    } else {                                                                                        \
      if ((D) <= 64) KERNEL<1, 1><<<grid, 256, 0, s>>>(__VA_ARGS__);                                \
      else if ((D) <= 128) KERNEL<1, 2><<<grid, 256, 0, s>>>(__VA_ARGS__);                          \
      else if ((D) <= 256) KERNEL<1, 4><<<grid, 256, 0, s>>>(__VA_ARGS__);                          \
      else if ((D) <= 512) KERNEL<1, 8><<<grid, 256, 0, s>>>(__VA_ARGS__);                          \
      else KERNEL<1, 16><<<grid, 256, 0, s>>>(__VA_ARGS__);                                         \
    }                                                                                               \
  } while (0)

extern "C" int sbr_score_cos_fwd(const float* U, const float* I, float* out, float* cos_raw, float* u_stat, float* i_stat, long B,
                                 int N, int D, float mu, float eps, void* stream) {
  if (B == 0 || N == 0) return SBR_OK;
  SBR_REQUIRE(U && I && out && cos_raw && u_stat && i_stat, "sbr_score_cos_fwd: null operand");
  SBR_REQUIRE(B > 0 && N > 0 && D >= 1 && eps > 0.f, "sbr_score_cos_fwd: needs B, N, D >= 1 and eps > 0");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)sbr_cdiv(B, 4);
  if (D > 1024) {
    score_cos_fwd_wide_kernel<<<grid, 256, 0, s>>>(U, I, out, cos_raw, u_stat, i_stat, B, N, D, mu, eps);
  } else {
    const bool vec = cos_vec_ok(D, U, I, nullptr, nullptr);
    SBR_COS_DISPATCH(score_cos_fwd_kernel, vec, D, U, I, out, cos_raw, u_stat, i_stat, B, N, D, mu, eps);
  }
  SBR_CHECK_LAUNCH("sbr_score_cos_fwd");
  return SBR_OK;
}

extern "C" int sbr_score_cos_bwd(const float* G, const float* U, const float* I, const float* cos_raw, const float* u_stat,
                                 const float* i_stat, float* dU, float* dI, long B, int N, int D, float mu, void* stream) {
  if (B == 0 || N == 0 || (!dU && !dI)) return SBR_OK;
  SBR_REQUIRE(G && U && I && cos_raw && u_stat && i_stat, "sbr_score_cos_bwd: null operand");
  SBR_REQUIRE(B > 0 && N > 0 && D >= 1, "sbr_score_cos_bwd: needs B, N, D >= 1");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)sbr_cdiv(B, 4);
  if (D > 1024) {
    score_cos_bwd_wide_kernel<<<grid, 256, 0, s>>>(G, U, I, cos_raw, u_stat, i_stat, dU, dI, B, N, D, mu);
  } else {
    const bool vec = cos_vec_ok(D, U, I, dU, dI);
    SBR_COS_DISPATCH(score_cos_bwd_kernel, vec, D, G, U, I, cos_raw, u_stat, i_stat, dU, dI, B, N, D, mu);
  }
  SBR_CHECK_LAUNCH("sbr_score_cos_bwd");
  return SBR_OK;
}

extern "C" int sbr_floor_scores(float* scores, long n, long n_cols, long ld, float mu, void* stream) {
  if (n == 0 || n_cols == 0) return SBR_OK;
  SBR_REQUIRE(scores && n > 0 && n_cols > 0 && ld >= n_cols, "sbr_floor_scores: needs a [n, n_cols] matrix with ld >= n_cols");
  const long total = n * n_cols;
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  floor_scores_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(scores, n, n_cols, ld, mu);
  SBR_CHECK_LAUNCH("sbr_floor_scores");
  return SBR_OK;
}
