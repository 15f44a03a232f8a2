// ProtoMF's shifted cosine similarity to a set of prototypes (algorithms/sgd_alg.py:48-59, compute_shifted_cosine_sim, as used by
// UProtoMF / IProtoMF / UIProtoMF, sgd_alg.py:380-399, 482-510) with the embedding lookup in front of it and the two arg-min
// regularisers behind it, forward and backward:
//     e = W[rows[j], :]      sim[j, p] = clamp(1 + e^ . p^, 0, 2),  x^ = x / max(|x|, 1e-12)                       (F.normalize's eps)
//     proto_loss = mean_p min_j (2 - sim[j, p])          batch_loss = mean_j min_p (2 - sim[j, p])                  (sgd_alg.py:394-399)
//
// Arithmetic: fp32 FMA throughout. The raw dot products e . P[p] are accumulated first and divided by the product of the two clamped norms
// (max(|x|, eps), saved for the backward pass) afterwards; column and loss sums that cross workgroups are double.
//
// Tie rule: a minimum attained more than once goes to the LOWEST index — the lowest prototype p for a row minimum, the lowest row j for a
// column minimum. The compared values are the fp32 distances 2 - sim themselves (the subtraction rounds for sim < 1, so two different
// similarities may tie as distances, as they do in the reference).
//
// Built on the 64 x 64 fp32 tile skeleton (csrc/tile64_f32.h; DESIGN.md has the work-item map, the LDS layout and the fixed-order rule).
// What crosses workgroups here: the column minimum is taken per workgroup over its own rows (in LDS), written as one partial per
// workgroup, and picked over the partials in workgroup order by one workgroup; the row-minimum sum is one double per workgroup, added
// in workgroup order; dP is written as one partial [P, D] per row split and folded in split order. The number of workgroups / splits
// depends on (R, D, P) only, never on the device. Unlike its two siblings this file keeps one 4 x 4 block per thread and walks the tiles:
//   forward   C[j, p] = sum_d e[j, d] P[p, d]      rows gathered straight from the table into LDS (the lookup is never materialised);
//                                                  the squared row norms are summed on the way in. P > 64: the prototype tiles are
//                                                  walked inside the row tile, the row tile comes back through the cache.
//   dE        C[j, d] = sum_p g'[j, p] P^[p, d]    g' = (G - w_batch/R [p = argmin_p] - w_proto/P [j = argmin_j]) where the clamp passes
//   dP        C[p, d] = sum_j g'[j, p] e^[j, d]    split over row ranges, partials folded in order
// followed by the projection terms of F.normalize's gradient ( - x^ (x^ . g) / |x| ), which need the row sums sum_p g' cos and the column
// sums sum_j g' cos: both are summed while g' is staged.
#include "tile64_f32.h"

namespace {

constexpr int PS_MAX_D = T64_MAX_D, PS_MAX_P = T64_MAX_N;
constexpr int PS_MAX_WG = 256;      // forward workgroups = column-minimum partials
constexpr int PS_MAX_SPLIT = 256;   // dP row splits (times D tiles times P tiles workgroups)

static inline int ps_fwd_wgs(long R) { return t64_wgs(R, PS_MAX_WG); }
static inline int ps_splits(long R, int D, int NP) {
  int s = PS_MAX_SPLIT / (t64_tiles(D) * t64_tiles(NP));
  const int t = t64_tiles(R);
  if (s > t) s = t;
  return s < 1 ? 1 : s;
}

// forward workspace: [wg doubles: row-minimum sums][2 * PS_MAX_P floats: prototype stats][wg * P floats][wg * P ints]
static inline size_t ps_fwd_ws_bytes(long R, int NP) {
  const size_t wg = (size_t)ps_fwd_wgs(R);
  return wg * sizeof(double) + 2 * PS_MAX_P * sizeof(float) + wg * NP * (sizeof(float) + sizeof(int));
}
// backward workspace: [splits * P * D floats: dP partials][splits * P floats: column sums of g' cos]
static inline size_t ps_bwd_ws_bytes(long R, int D, int NP) {
  return (size_t)ps_splits(R, D, NP) * NP * ((size_t)D + 1) * sizeof(float);
}

// (v, i) <- the smaller of (v, i) and (v2, i2); equal values: the lower index
__device__ __forceinline__ void ps_take_min(float& v, int& i, float v2, int i2) {
  if (v2 < v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

template <bool STATS>
__global__ __launch_bounds__(256) void ps_fwd_kernel(const float* __restrict__ W, long ldw, const int* __restrict__ rows, long R, int D,
                                                     const float* __restrict__ P, int NP, const float* __restrict__ pstat,
                                                     float* __restrict__ sim_out, float* __restrict__ cos_raw, float* __restrict__ row_stat,
                                                     int* __restrict__ row_best, float* __restrict__ part_cv, int* __restrict__ part_cj,
                                                     double* __restrict__ part_rs, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_rnc[T64_T];
  __shared__ float s_colv[PS_MAX_P];
  __shared__ int s_colj[PS_MAX_P];
  __shared__ float s_wv[4][T64_T];
  __shared__ int s_wj[4][T64_T];
  __shared__ float s_rowdis[T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4, lane = t & 63, wave = t >> 6;
  const int sk = t & 31, sr = t >> 5;                 // staging of a transposed tile: k within the chunk, first of 8 rows (stride 8)
  if (STATS) {
    for (int p = t; p < PS_MAX_P; p += 256) { s_colv[p] = INFINITY; s_colj[p] = INT_MAX; }
  }
  double rowsum = 0.0;                                // thread 0: sum of this workgroup's row minima, in tile order
  const int n_pt = (NP + T64_T - 1) / T64_T;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    const float* rp[8];
    t64_row_ptrs(rp, W, ldw, rows, j0, R, sr);
    float ss[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) ss[q] = 0.f;
    float rbv[4];
    int rbp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { rbv[i] = INFINITY; rbp[i] = INT_MAX; }
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
      float cbv[4];
      int cbj[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) { cbv[c] = INFINITY; cbj[c] = INT_MAX; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long j = j0 + 4 * rg + i;
        const float enc = s_rnc[4 * rg + i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int p = pt * T64_T + 4 * cg + c;
          if (j < R && p < NP) {
            const float cs = acc[i][c] / (enc * pnc[c]);          // both factors >= 1e-12: the product is a normal number
            const float x = 1.f + cs;
            const float sim = x < 0.f ? 0.f : (x > 2.f ? 2.f : x);       // torch.clamp: a NaN stays
            sim_out[j * NP + p] = sim;
            if (cos_raw) cos_raw[j * NP + p] = cs;
            if (STATS) {
              const float dis = 2.f - sim;
              if (dis < rbv[i]) { rbv[i] = dis; rbp[i] = p; }             // p ascends within a thread: the first minimum stays
              if (dis < cbv[c]) { cbv[c] = dis; cbj[c] = (int)j; }        // and so does j
            }
          }
        }
      }
      if (STATS) {
        // column minima of this prototype tile: over the row groups of a wave (lane bits 4, 5), over the waves, into the running minimum
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int o = 16; o <= 32; o <<= 1) {
            const float v2 = __shfl_xor(cbv[c], o, 64);
            const int j2 = __shfl_xor(cbj[c], o, 64);
            ps_take_min(cbv[c], cbj[c], v2, j2);
          }
          if (lane < 16) { s_wv[wave][4 * cg + c] = cbv[c]; s_wj[wave][4 * cg + c] = cbj[c]; }
        }
        __syncthreads();
        if (t < T64_T) {
          const int p = pt * T64_T + t;
          if (p < NP) {
            float v = s_colv[p];
            int j = s_colj[p];
#pragma unroll
            for (int w = 0; w < 4; ++w) ps_take_min(v, j, s_wv[w][t], s_wj[w][t]);
            s_colv[p] = v; s_colj[p] = j;
          }
        }
        __syncthreads();
      }
    }
    if (STATS) {
      // row minima: over the 16 column groups of a row group (lane bits 0 .. 3)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float v2 = __shfl_xor(rbv[i], o, 64);
          const int p2 = __shfl_xor(rbp[i], o, 64);
          ps_take_min(rbv[i], rbp[i], v2, p2);
        }
        if (cg == 0) {
          const long j = j0 + 4 * rg + i;
          if (j < R) row_best[j] = rbp[i];
          s_rowdis[4 * rg + i] = j < R ? rbv[i] : 0.f;
        }
      }
      __syncthreads();
      if (wave == 0) {
        const double v = sbr_wave_sum_d((double)s_rowdis[lane]);
        if (t == 0) rowsum += v;
      }
      __syncthreads();
    }
  }
  if (STATS) {
    __syncthreads();
    for (int p = t; p < NP; p += 256) {
      part_cv[(long)blockIdx.x * NP + p] = s_colv[p];
      part_cj[(long)blockIdx.x * NP + p] = s_colj[p];
    }
    if (t == 0) part_rs[blockIdx.x] = rowsum;
  }
}

// the ordered pick over the workgroups' column minima and the two regulariser scalars (one workgroup)
__global__ __launch_bounds__(256) void ps_fin_kernel(const float* __restrict__ part_cv, const int* __restrict__ part_cj,
                                                     const double* __restrict__ part_rs, int nb, int NP, long R,
                                                     float* __restrict__ col_best_val, int* __restrict__ col_best_row,
                                                     float* __restrict__ proto_loss, float* __restrict__ batch_loss) {
  __shared__ float s_v[PS_MAX_P];
  const int t = threadIdx.x;
  for (int p = t; p < NP; p += 256) {
    float v = INFINITY;
    int j = INT_MAX;
#pragma unroll 8
    for (int b = 0; b < nb; ++b) ps_take_min(v, j, part_cv[(long)b * NP + p], part_cj[(long)b * NP + p]);
    col_best_val[p] = v;
    col_best_row[p] = j;
    s_v[p] = v;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int p = 0; p < NP; ++p) s += (double)s_v[p];
    *proto_loss = (float)(s / NP);
  }
  if (t == 64) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part_rs[b];
    *batch_loss = (float)(s / (double)R);
  }
}

// g'[j, p] and the un-clamped cosine it belongs to
struct PsGrad {
  const float* G;
  const float* cos_raw;
  const int* row_best;
  const int* col_best_row;
  float w_proto, w_batch;       // upstream gradient of the regulariser x 1 / P, x 1 / R
  int NP;
  __device__ __forceinline__ float at(long j, int p, float& cs) const {
    cs = cos_raw[j * NP + p];
    const float x = 1.f + cs;
    float g = G[j * NP + p];
    if (row_best[j] == p) g -= w_batch;
    if (col_best_row[p] == (int)j) g -= w_proto;
    return (x >= 0.f && x <= 2.f) ? g : 0.f;        // torch.clamp passes the gradient on the closed interval
  }
};

__device__ __forceinline__ PsGrad ps_grad(const float* G, const float* g_proto, const float* g_batch, const float* cos_raw,
                                          const int* row_best, const int* col_best_row, long R, int NP) {
  PsGrad g;
  g.G = G; g.cos_raw = cos_raw; g.row_best = row_best; g.col_best_row = col_best_row; g.NP = NP;
  g.w_proto = g_proto ? *g_proto / (float)NP : 0.f;
  g.w_batch = g_batch ? *g_batch / (float)R : 0.f;
  return g;
}

// dE[j, :] = (sum_p g' P^[p, :] - [|e| >= eps] e^[j, :] sum_p g' cos) / max(|e|, eps)
__global__ __launch_bounds__(256) void ps_bwd_de_kernel(const float* __restrict__ G, const float* __restrict__ g_proto,
                                                        const float* __restrict__ g_batch, const float* __restrict__ W, long ldw,
                                                        const int* __restrict__ rows, long R, int D, const float* __restrict__ P, int NP,
                                                        const float* __restrict__ cos_raw, const float* __restrict__ row_stat,
                                                        const float* __restrict__ pstat, const int* __restrict__ row_best,
                                                        const int* __restrict__ col_best_row, float* __restrict__ dE, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_S[T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int sk = t & 31, sr = t >> 5;                 // g' tile, transposed: prototype within the chunk, first of 8 rows
  const int bc = t & 63, bk = t >> 6;                 // prototype tile, as stored: column, first of 8 k (stride 4)
  const PsGrad gr = ps_grad(G, g_proto, g_batch, cos_raw, row_best, col_best_row, R, NP);
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
__global__ __launch_bounds__(256) void ps_bwd_dp_kernel(const float* __restrict__ G, const float* __restrict__ g_proto,
                                                        const float* __restrict__ g_batch, const float* __restrict__ W, long ldw,
                                                        const int* __restrict__ rows, long R, int D, int NP,
                                                        const float* __restrict__ cos_raw, const float* __restrict__ row_stat,
                                                        const int* __restrict__ row_best, const int* __restrict__ col_best_row,
                                                        float* __restrict__ part, float* __restrict__ part_t, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_T[4][T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int bc = t & 63, bk = t >> 6;                 // both operands as stored: column, first of 8 k (stride 4)
  const PsGrad gr = ps_grad(G, g_proto, g_batch, cos_raw, row_best, col_best_row, R, NP);
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
struct PsFoldEpi {
  static constexpr bool kColumnSums = true;
  const float* P;
  const float* pstat;
  __device__ __forceinline__ float operator()(long e, int p, float s, float tt) const {
    const float nc = pstat[2 * p], flag = pstat[2 * p + 1];
    return fmaf(-(flag * (P[e] / nc)), tt, s) / nc;
  }
};

inline bool ps_shape_ok(int D, int NP) { return D >= 1 && D <= PS_MAX_D && NP >= 2 && NP <= PS_MAX_P; }

}  // namespace

extern "C" long sbr_proto_sim_workspace(long R, int D, int n_proto, int backward) {
  if (R <= 0 || !ps_shape_ok(D, n_proto)) return 0;
  return (long)(backward ? ps_bwd_ws_bytes(R, D, n_proto) : ps_fwd_ws_bytes(R, n_proto));
}

extern "C" int sbr_proto_sim_fwd(const float* W, long ldw, const int* rows, long R, int D, const float* P, int n_proto, float* sim_out,
                                 float* cos_raw, float* row_stat, float* proto_stat, int* row_best, float* col_best_val,
                                 int* col_best_row, float* proto_loss, float* batch_loss, void* workspace, long workspace_bytes,
                                 void* stream) {
  SBR_REQUIRE(ps_shape_ok(D, n_proto), "sbr_proto_sim_fwd: needs 1 <= D <= %d and 2 <= n_proto <= %d (got D = %d, n_proto = %d)", PS_MAX_D,
              PS_MAX_P, D, n_proto);
  if (R == 0) return SBR_OK;
  SBR_REQUIRE(R > 0 && R < INT_MAX && ldw >= D, "sbr_proto_sim_fwd: needs 0 <= R < 2^31 and ldw >= D");
  SBR_REQUIRE(W && P && sim_out && workspace, "sbr_proto_sim_fwd: null operand");
  const bool stats = row_best || col_best_val || col_best_row || proto_loss || batch_loss;
  SBR_REQUIRE(!stats || (row_best && col_best_val && col_best_row && proto_loss && batch_loss),
              "sbr_proto_sim_fwd: the arg-min outputs and the two losses come together (all or none)");
  SBR_REQUIRE(workspace_bytes >= (long)ps_fwd_ws_bytes(R, n_proto), "sbr_proto_sim_fwd: workspace of %ld bytes, needs %ld", workspace_bytes,
              (long)ps_fwd_ws_bytes(R, n_proto));
  hipStream_t s = (hipStream_t)stream;
  const int nb = ps_fwd_wgs(R), n_tiles = t64_tiles(R);
  double* part_rs = (double*)workspace;
  float* pstat = (float*)(part_rs + nb);
  float* part_cv = pstat + 2 * PS_MAX_P;
  int* part_cj = (int*)(part_cv + (size_t)nb * n_proto);
  t64_norm_kernel<<<sbr_cdiv(n_proto, 4), 256, 0, s>>>(P, n_proto, D, pstat, proto_stat);
  if (stats) {
    ps_fwd_kernel<true><<<nb, 256, 0, s>>>(W, ldw, rows, R, D, P, n_proto, pstat, sim_out, cos_raw, row_stat, row_best, part_cv, part_cj,
                                           part_rs, n_tiles);
    ps_fin_kernel<<<1, 256, 0, s>>>(part_cv, part_cj, part_rs, nb, n_proto, R, col_best_val, col_best_row, proto_loss, batch_loss);
  } else {
    ps_fwd_kernel<false><<<nb, 256, 0, s>>>(W, ldw, rows, R, D, P, n_proto, pstat, sim_out, cos_raw, row_stat, nullptr, nullptr, nullptr,
                                            nullptr, n_tiles);
  }
  SBR_CHECK_LAUNCH("sbr_proto_sim_fwd");
  return SBR_OK;
}

extern "C" int sbr_proto_sim_bwd(const float* G, const float* g_proto, const float* g_batch, const float* W, long ldw, const int* rows,
                                 long R, int D, const float* P, int n_proto, const float* cos_raw, const float* row_stat,
                                 const float* proto_stat, const int* row_best, const int* col_best_row, float* dE, float* dP,
                                 void* workspace, long workspace_bytes, void* stream) {
  SBR_REQUIRE(ps_shape_ok(D, n_proto), "sbr_proto_sim_bwd: needs 1 <= D <= %d and 2 <= n_proto <= %d (got D = %d, n_proto = %d)", PS_MAX_D,
              PS_MAX_P, D, n_proto);
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {
    if (dP) {
      hipError_t e = hipMemsetAsync(dP, 0, (size_t)n_proto * D * sizeof(float), s);
      SBR_REQUIRE(e == hipSuccess, "sbr_proto_sim_bwd: memset failed: %s", hipGetErrorString(e));
    }
    return SBR_OK;
  }
  SBR_REQUIRE(R > 0 && R < INT_MAX && ldw >= D, "sbr_proto_sim_bwd: needs 0 <= R < 2^31 and ldw >= D");
  SBR_REQUIRE(G && W && P && cos_raw && row_stat && proto_stat && row_best && col_best_row, "sbr_proto_sim_bwd: null operand");
  const int n_tiles = t64_tiles(R);
  if (dE) {
    const int nb = n_tiles < 8192 ? n_tiles : 8192;
    ps_bwd_de_kernel<<<nb, 256, 0, s>>>(G, g_proto, g_batch, W, ldw, rows, R, D, P, n_proto, cos_raw, row_stat, proto_stat, row_best,
                                        col_best_row, dE, n_tiles);
  }
  if (dP) {
    SBR_REQUIRE(workspace && workspace_bytes >= (long)ps_bwd_ws_bytes(R, D, n_proto), "sbr_proto_sim_bwd: workspace of %ld bytes, needs %ld",
                workspace_bytes, (long)ps_bwd_ws_bytes(R, D, n_proto));
    const int n_split = ps_splits(R, D, n_proto);
    float* part = (float*)workspace;
    float* part_t = part + (size_t)n_split * n_proto * D;
    const dim3 grid(n_split, t64_tiles(D), t64_tiles(n_proto));
    ps_bwd_dp_kernel<<<grid, 256, 0, s>>>(G, g_proto, g_batch, W, ldw, rows, R, D, n_proto, cos_raw, row_stat, row_best, col_best_row, part,
                                          part_t, n_tiles);
    t64_fold_kernel<<<sbr_cdiv((long)n_proto * D, 256), 256, 0, s>>>(part, part_t, n_split, n_proto, D, PsFoldEpi{P, proto_stat}, dP);
  }
  SBR_CHECK_LAUNCH("sbr_proto_sim_bwd");
  return SBR_OK;
}
