// The simplified ProtoMF family's prototype side (algorithms/sgd_alg.py:643-850: UProtoMFs / IProtoMFs / UIProtoMFs): the plain cosine
// similarity to the prototypes (compute_cosine_sim, sgd_alg.py:62-73) with the embedding lookup in front of it and, in the score form,
// the ReLU on the other entity's weights (sgd_alg.py:683, 739, 808, 814) and the dot over the prototypes (sgd_alg.py:687, 750, 823-824)
// behind it, forward and backward:
//     e = W[rows[j], :]      cos[j, p] = clamp(e^ . P^_p, -1, 1),  x^ = x / max(|x|, 1e-12)                            (F.normalize's eps)
//     w[j, f, :] = Wt[widx[j fan + f], :]          out[j, f] = sum_p cos[j, p] max(w[j, f, p], 0)
// There are no regularisers in this family, so nothing here takes a minimum.
//
// Arithmetic: fp32 FMA throughout, as in csrc/proto_sim.hip: the raw dot products are accumulated first and divided by the product of the
// two clamped norms (saved for the backward pass) afterwards. One form only, no float atomics: the only sum that crosses workgroups is dP,
// written as one partial [P, D] per row split and folded in split order in double (t64_fold_kernel). The number of splits depends on
// (R, D, P) only, never on the device.
//
// Built on the 64 x 64 fp32 tile skeleton (csrc/tile64_f32.h; DESIGN.md has the work-item map):
//   forward   C[j, p] = sum_d e[j, d] P[p, d]      rows gathered straight from the table into LDS, the squared row norms summed on the
//                                                  way in. Score form: the clamped cosines of the tile go to LDS and every thread takes
//                                                  the outputs (j, f) = t, t + 256, ... of the tile: the weight row is read from the
//                                                  table, the ReLU applied in registers, four interleaved sums over p.
//                                                  P > 64: the prototype tiles are walked inside the row tile and out[j, f]
//                                                  takes the partial dots in tile order (the same thread owns an output in
//                                                  every tile).
//   dE        C[j, d] = sum_p g'[j, p] P^[p, d]    g' = dcos where the clamp passes (the closed interval [-1, 1], as torch.clamp)
//   dP        C[p, d] = sum_j g'[j, p] e^[j, d]    split over row ranges, partials folded in order
// followed by the projection terms of F.normalize's gradient and the eps flags, exactly as in ps_bwd_de_kernel / ps_bwd_dp_kernel /
// PsFoldEpi. dcos is pluggable (PqGivenGrad: a given G_cos [R, P]; PqScoreGrad: sum_f g[j, f] max(w[j, f, p], 0), the weight rows read
// again from the table); the weight-row gradient dWrows[j fan + f, p] = g[j, f] cos[j, p] [w > 0] is one element-wise pass.
//
// Saved by the forward for the backward: the un-clamped cosine [R, P], {max(|e|, eps), |e| >= eps} per row, the same per prototype: what
// sbr_proto_sim_fwd keeps. The gathered (and relu'd) weights are never written.
#include "tile64_f32.h"

namespace {

constexpr int PQ_MAX_D = T64_MAX_D, PQ_MAX_P = T64_MAX_N;
constexpr int PQ_MAX_WG = 8192;     // forward / dE workgroups: a grid-stride loop over the row tiles beyond it
constexpr int PQ_MAX_SPLIT = 256;   // dP row splits (times D tiles times P tiles workgroups)
constexpr int PQ_LDC = T64_T + 1;   // row stride of the cosine tile in LDS: a thread walks a row, neighbours hold other rows

static inline int pq_splits(long R, int D, int NP) {
  int s = PQ_MAX_SPLIT / (t64_tiles(D) * t64_tiles(NP));
  const int t = t64_tiles(R);
  if (s > t) s = t;
  return s < 1 ? 1 : s;
}
// forward workspace: [2 * PQ_MAX_P floats: prototype stats]
static inline size_t pq_fwd_ws_bytes() { return 2 * PQ_MAX_P * sizeof(float); }
// backward workspace: [splits * P * D floats: dP partials][splits * P floats: column sums of g' cos]
static inline size_t pq_bwd_ws_bytes(long R, int D, int NP) { return (size_t)pq_splits(R, D, NP) * NP * ((size_t)D + 1) * sizeof(float); }

// torch.clamp(x, -1, 1) and torch.relu: a NaN stays a NaN
__device__ __forceinline__ float pq_clamp(float x) { return x < -1.f ? -1.f : (x > 1.f ? 1.f : x); }
__device__ __forceinline__ float pq_relu(float w) { return w <= 0.f ? 0.f : w; }

template <bool SCORE>
__global__ __launch_bounds__(256) void pq_fwd_kernel(const float* __restrict__ W, long ldw, const int* __restrict__ rows, long R, int D,
                                                     const float* __restrict__ P, int NP, const float* __restrict__ pstat,
                                                     const float* __restrict__ Wt, long ldwt, const int* __restrict__ widx, int fan,
                                                     float* __restrict__ cos_out, float* __restrict__ out, float* __restrict__ cos_raw,
                                                     float* __restrict__ row_stat, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_rnc[T64_T];
  __shared__ float s_cos[SCORE ? T64_T * PQ_LDC : 1];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int sk = t & 31, sr = t >> 5;                 // staging of a transposed tile: k within the chunk, first of 8 rows (stride 8)
  const int n_pt = (NP + T64_T - 1) / T64_T;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    const float* rp[8];
    t64_row_ptrs(rp, W, ldw, rows, j0, R, sr);
    float ss[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) ss[q] = 0.f;
    for (int pt = 0; pt < n_pt; ++pt) {
      float acc[4][4];
      t64_zero(acc);
      for (int d0 = 0; d0 < D; d0 += T64_KC) {
        t64_stage_rows_t(As, rp, d0 + sk, D, sk, sr, ss, pt == 0);
        t64_stage_tile_t(Bs, P, pt, NP, d0 + sk, D, sk, sr);
        __syncthreads();
        t64_mma(As, Bs, rg, cg, acc);
        __syncthreads();
      }
      if (pt == 0) {
        // the 32 lanes that share sr hold the squared norm of rows sr + 8 q in 32 pieces
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float v = t64_half_sum<true>(ss[q]);
          if (sk == 0) {
            float nc, flag;
            t64_stats(v, nc, flag);
            s_rnc[sr + 8 * q] = nc;
            const long j = j0 + sr + 8 * q;
            if (row_stat && j < R) { row_stat[2 * j] = nc; row_stat[2 * j + 1] = flag; }
          }
        }
        __syncthreads();
      }
      float pnc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int p = pt * T64_T + 4 * cg + c;
        pnc[c] = p < NP ? pstat[2 * p] : 1.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long j = j0 + 4 * rg + i;
        const float enc = s_rnc[4 * rg + i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int p = pt * T64_T + 4 * cg + c;
          float cc = 0.f;
          if (j < R && p < NP) {
            const float cs = acc[i][c] / (enc * pnc[c]);          // both factors >= 1e-12: the product is a normal number
            cc = pq_clamp(cs);
            if (cos_out) cos_out[j * NP + p] = cc;
            if (cos_raw) cos_raw[j * NP + p] = cs;
          }
          if (SCORE) s_cos[(4 * rg + i) * PQ_LDC + 4 * cg + c] = cc;
        }
      }
      if (SCORE) {
        __syncthreads();
        const int pw = NP - pt * T64_T < T64_T ? NP - pt * T64_T : T64_T;
        long rows_here = R - j0;
        if (rows_here > T64_T) rows_here = T64_T;
        const long n_out = rows_here * fan;                       // outputs of this tile: (row, f), f fastest
        for (long o = t; o < n_out; o += 256) {
          const int jl = (int)(o / fan);
          const long wi = j0 * fan + o;                           // = j fan + f
          const float* wr = Wt + (long)(widx ? widx[wi] : wi) * ldwt + pt * T64_T;
          const float* cr = s_cos + jl * PQ_LDC;
          float s4[4] = {0.f, 0.f, 0.f, 0.f};                     // four interleaved partial sums over p, a fixed order
          int p = 0;
          for (; p + 4 <= pw; p += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s4[q] = fmaf(cr[p + q], pq_relu(wr[p + q]), s4[q]);
          }
          for (int q = 0; p < pw; ++p, ++q) s4[q] = fmaf(cr[p], pq_relu(wr[p]), s4[q]);
          const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
          out[wi] = pt == 0 ? s : out[wi] + s;
        }
        __syncthreads();
      }
    }
  }
}

// dcos[j, p] where the clamp passes, and the un-clamped cosine it belongs to: a given G_cos [R, P] ...
struct PqGivenGrad {
  const float* G;
  const float* cos_raw;
  int NP;
  __device__ __forceinline__ float at(long j, int p, float& cs) const {
    cs = cos_raw[j * NP + p];
    const float g = G[j * NP + p];
    return (cs >= -1.f && cs <= 1.f) ? g : 0.f;       // torch.clamp passes the gradient on the closed interval
  }
};
// ... or sum_f g[j, f] max(w[j, f, p], 0) of the score form, f ascending
struct PqScoreGrad {
  const float* g;
  const float* cos_raw;
  const float* Wt;
  const int* widx;
  long ldwt;
  int fan, NP;
  __device__ __forceinline__ float at(long j, int p, float& cs) const {
    cs = cos_raw[j * NP + p];
    float s = 0.f;
    for (int f = 0; f < fan; ++f) {
      const long wi = j * fan + f;
      s = fmaf(g[wi], pq_relu(Wt[(long)(widx ? widx[wi] : wi) * ldwt + p]), s);
    }
    return (cs >= -1.f && cs <= 1.f) ? s : 0.f;
  }
};

// dE[j, :] = (sum_p g' P^[p, :] - [|e| >= eps] e^[j, :] sum_p g' cos) / max(|e|, eps)
template <class Grad>
__global__ __launch_bounds__(256) void pq_bwd_de_kernel(const Grad gr, const float* __restrict__ W, long ldw, const int* __restrict__ rows,
                                                        long R, int D, const float* __restrict__ P, int NP,
                                                        const float* __restrict__ row_stat, const float* __restrict__ pstat,
                                                        float* __restrict__ dE, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_S[T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int sk = t & 31, sr = t >> 5;                 // g' tile, transposed: prototype within the chunk, first of 8 rows
  const int bc = t & 63, bk = t >> 6;                 // prototype tile, as stored: column, first of 8 k (stride 4)
  const int n_dt = (D + T64_T - 1) / T64_T;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    for (int dt = 0; dt < n_dt; ++dt) {
      float acc[4][4];
      t64_zero(acc);
      float S[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) S[q] = 0.f;
      for (int p0 = 0; p0 < NP; p0 += T64_KC) {
        const int p = p0 + sk;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const long j = j0 + sr + 8 * q;
          float v = 0.f;
          if (j < R && p < NP) {
            float cs;
            v = gr.at(j, p, cs);
            S[q] = fmaf(v, cs, S[q]);
          }
          As[sk * T64_LD + sr + 8 * q] = v;
        }
        t64_stage_chunk<true>(Bs, P, pstat, p0, NP, dt, D, bc, bk);
        __syncthreads();
        t64_mma(As, Bs, rg, cg, acc);
        __syncthreads();
      }
      if (dt == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float v = t64_half_sum<true>(S[q]);
          if (sk == 0) s_S[sr + 8 * q] = v;
        }
        __syncthreads();
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long j = j0 + 4 * rg + i;
        if (j >= R) continue;
        const float nc = row_stat[2 * j], flag = row_stat[2 * j + 1];
        const float Sj = s_S[4 * rg + i];
        const float* erow = W + (long)(rows ? rows[j] : j) * ldw;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int d = dt * T64_T + 4 * cg + c;
          if (d < D) dE[j * D + d] = fmaf(-(flag * (erow[d] / nc)), Sj, acc[i][c]) / nc;
        }
      }
    }
    __syncthreads();                                  // s_S belongs to the next tile from here
  }
}

// one row split's share of sum_j g'[j, p] e^[j, d] (tile blockIdx.z of p, blockIdx.y of d) and of sum_j g'[j, p] cos[j, p]
template <class Grad>
__global__ __launch_bounds__(256) void pq_bwd_dp_kernel(const Grad gr, const float* __restrict__ W, long ldw, const int* __restrict__ rows,
                                                        long R, int D, int NP, const float* __restrict__ row_stat,
                                                        float* __restrict__ part, float* __restrict__ part_t, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_T[4][T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int bc = t & 63, bk = t >> 6;                 // both operands as stored: column, first of 8 k (stride 4)
  const int split = blockIdx.x, dt = blockIdx.y, pt = blockIdx.z;
  const int per = (n_tiles + gridDim.x - 1) / gridDim.x;
  const long jlo = (long)split * per * T64_T;
  long jhi = jlo + (long)per * T64_T;
  if (jhi > R) jhi = R;
  const int p = pt * T64_T + bc, d = dt * T64_T + bc;
  float acc[4][4];
  t64_zero(acc);
  float T = 0.f;
  for (long jc = jlo; jc < jhi; jc += T64_KC) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = bk + 4 * q;
      const long j = jc + k;
      float a = 0.f, b = 0.f;
      if (j < jhi) {
        if (p < NP) {
          float cs;
          const float g = gr.at(j, p, cs);
          T = fmaf(g, cs, T);
          a = g;
        }
        if (d < D) b = W[(long)(rows ? rows[j] : j) * ldw + d] / row_stat[2 * j];
      }
      As[k * T64_LD + bc] = a;
      Bs[k * T64_LD + bc] = b;
    }
    __syncthreads();
    t64_mma(As, Bs, rg, cg, acc);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pp = pt * T64_T + 4 * rg + i;
    if (pp >= NP) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int dd = dt * T64_T + 4 * cg + c;
      if (dd < D) part[((long)split * NP + pp) * D + dd] = acc[i][c];
    }
  }
  if (dt == 0) {
    s_T[bk][bc] = T;
    __syncthreads();
    if (t < T64_T && p < NP) part_t[(long)split * NP + p] = (s_T[0][t] + s_T[1][t]) + (s_T[2][t] + s_T[3][t]);
  }
}

// dP[p, d] = (sum over splits - [|P[p]| >= eps] P^[p, d] sum_j g' cos) / max(|P[p]|, eps), the splits added in order (t64_fold_kernel)
struct PqFoldEpi {
  static constexpr bool kColumnSums = true;
  const float* P;
  const float* pstat;
  __device__ __forceinline__ float operator()(long e, int p, float s, float tt) const {
    const float nc = pstat[2 * p], flag = pstat[2 * p + 1];
    return fmaf(-(flag * (P[e] / nc)), tt, s) / nc;
  }
};

// dWrows[j fan + f, p] = g[j, f] clamp(cos)[j, p] [w[j, f, p] > 0]: zero at w == 0, as torch's ReLU
__global__ __launch_bounds__(256) void pq_bwd_dw_kernel(const float* __restrict__ g, const float* __restrict__ cos_raw,
                                                        const float* __restrict__ Wt, long ldwt, const int* __restrict__ widx, int fan,
                                                        int NP, long n, float* __restrict__ dWrows) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += (long)gridDim.x * 256L) {
    const long wi = e / NP;
    const int p = (int)(e - wi * NP);
    const long j = wi / fan;
    const float w = Wt[(long)(widx ? widx[wi] : wi) * ldwt + p];
    dWrows[e] = w > 0.f ? g[wi] * pq_clamp(cos_raw[j * NP + p]) : 0.f;
  }
}

inline bool pq_shape_ok(int D, int NP) { return D >= 1 && D <= PQ_MAX_D && NP >= 2 && NP <= PQ_MAX_P; }

}  // namespace

extern "C" long sbr_proto_score_workspace(long R, int D, int n_proto, int backward) {
  if (R <= 0 || !pq_shape_ok(D, n_proto)) return 0;
  return (long)(backward ? pq_bwd_ws_bytes(R, D, n_proto) : pq_fwd_ws_bytes());
}

#define PQ_REQUIRE_SHAPE(who)                                                                                                          \
  SBR_REQUIRE(pq_shape_ok(D, n_proto) && fan >= 1, who ": needs 1 <= D <= %d, 2 <= n_proto <= %d and 1 <= fan (got D = %d, n_proto = %d, " \
              "fan = %d)", PQ_MAX_D, PQ_MAX_P, D, n_proto, fan)

extern "C" int sbr_proto_score_fwd(const float* W, long ldw, const int* rows, long R, int D, const float* P, int n_proto, const float* Wt,
                                   long ldwt, const int* widx, int fan, float* cos_out, float* out, float* cos_raw, float* row_stat,
                                   float* proto_stat, void* workspace, long workspace_bytes, void* stream) {
  PQ_REQUIRE_SHAPE("sbr_proto_score_fwd");
  if (R == 0) return SBR_OK;
  SBR_REQUIRE(R > 0 && R < INT_MAX && R * (long)fan < INT_MAX && ldw >= D,
              "sbr_proto_score_fwd: needs 0 <= R, R * fan < 2^31 and ldw >= D (got R = %ld, fan = %d)", R, fan);
  SBR_REQUIRE(W && P && workspace, "sbr_proto_score_fwd: null operand");
  SBR_REQUIRE(Wt ? (out && ldwt >= n_proto) : (cos_out && !out && !widx),
              "sbr_proto_score_fwd: the score form needs Wt, out and ldwt >= n_proto; the cosine form cos_out and neither out nor widx");
  SBR_REQUIRE(workspace_bytes >= (long)pq_fwd_ws_bytes(), "sbr_proto_score_fwd: workspace of %ld bytes, needs %ld", workspace_bytes,
              (long)pq_fwd_ws_bytes());
  hipStream_t s = (hipStream_t)stream;
  const int n_tiles = t64_tiles(R), nb = t64_wgs(R, PQ_MAX_WG);
  float* pstat = (float*)workspace;
  t64_norm_kernel<<<sbr_cdiv(n_proto, 4), 256, 0, s>>>(P, n_proto, D, pstat, proto_stat);
  if (Wt)
    pq_fwd_kernel<true><<<nb, 256, 0, s>>>(W, ldw, rows, R, D, P, n_proto, pstat, Wt, ldwt, widx, fan, cos_out, out, cos_raw, row_stat,
                                           n_tiles);
  else
    pq_fwd_kernel<false><<<nb, 256, 0, s>>>(W, ldw, rows, R, D, P, n_proto, pstat, nullptr, 0, nullptr, 1, cos_out, nullptr, cos_raw,
                                            row_stat, n_tiles);
  SBR_CHECK_LAUNCH("sbr_proto_score_fwd");
  return SBR_OK;
}

extern "C" int sbr_proto_score_bwd(const float* G, const float* W, long ldw, const int* rows, long R, int D, const float* P, int n_proto,
                                   const float* Wt, long ldwt, const int* widx, int fan, const float* cos_raw, const float* row_stat,
                                   const float* proto_stat, float* dE, float* dP, float* dWrows, void* workspace, long workspace_bytes,
                                   void* stream) {
  PQ_REQUIRE_SHAPE("sbr_proto_score_bwd");
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {
    if (dP) {
      hipError_t e = hipMemsetAsync(dP, 0, (size_t)n_proto * D * sizeof(float), s);
      SBR_REQUIRE(e == hipSuccess, "sbr_proto_score_bwd: memset failed: %s", hipGetErrorString(e));
    }
    return SBR_OK;
  }
  SBR_REQUIRE(R > 0 && R < INT_MAX && R * (long)fan < INT_MAX && ldw >= D,
              "sbr_proto_score_bwd: needs 0 <= R, R * fan < 2^31 and ldw >= D (got R = %ld, fan = %d)", R, fan);
  SBR_REQUIRE(G && W && P && cos_raw && row_stat && proto_stat, "sbr_proto_score_bwd: null operand");
  SBR_REQUIRE(Wt ? ldwt >= n_proto : (!dWrows && !widx),
              "sbr_proto_score_bwd: the score form needs Wt and ldwt >= n_proto; the cosine form has neither dWrows nor widx");
  const int n_tiles = t64_tiles(R), nb = t64_wgs(R, PQ_MAX_WG);
  const PqGivenGrad given{G, cos_raw, n_proto};
  const PqScoreGrad score{G, cos_raw, Wt, widx, ldwt, fan, n_proto};
  if (dWrows) {
    const long n = R * (long)fan * n_proto;
    const long blocks = sbr_cdiv(n, 256);
    pq_bwd_dw_kernel<<<(int)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>(G, cos_raw, Wt, ldwt, widx, fan, n_proto, n, dWrows);
  }
  if (dE) {
    if (Wt)
      pq_bwd_de_kernel<<<nb, 256, 0, s>>>(score, W, ldw, rows, R, D, P, n_proto, row_stat, proto_stat, dE, n_tiles);
    else
      pq_bwd_de_kernel<<<nb, 256, 0, s>>>(given, W, ldw, rows, R, D, P, n_proto, row_stat, proto_stat, dE, n_tiles);
  }
  if (dP) {
    SBR_REQUIRE(workspace && workspace_bytes >= (long)pq_bwd_ws_bytes(R, D, n_proto),
                "sbr_proto_score_bwd: workspace of %ld bytes, needs %ld", workspace_bytes, (long)pq_bwd_ws_bytes(R, D, n_proto));
    const int n_split = pq_splits(R, D, n_proto);
    float* part = (float*)workspace;
    float* part_t = part + (size_t)n_split * n_proto * D;
    const dim3 grid(n_split, t64_tiles(D), t64_tiles(n_proto));
    if (Wt)
      pq_bwd_dp_kernel<<<grid, 256, 0, s>>>(score, W, ldw, rows, R, D, n_proto, row_stat, part, part_t, n_tiles);
    else
      pq_bwd_dp_kernel<<<grid, 256, 0, s>>>(given, W, ldw, rows, R, D, n_proto, row_stat, part, part_t, n_tiles);
    t64_fold_kernel<<<sbr_cdiv((long)n_proto * D, 256), 256, 0, s>>>(part, part_t, n_split, n_proto, D, PqFoldEpi{P, proto_stat}, dP);
  }
  SBR_CHECK_LAUNCH("sbr_proto_score_bwd");
  return SBR_OK;
}
