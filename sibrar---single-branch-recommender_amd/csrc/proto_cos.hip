// The cosine-to-prototypes family: gathered table rows against a small prototype matrix, differentiated through F.normalize, with the
// embedding lookup fused in front. Two ops share everything up to the cosine and the whole backward:
//   ProtoMF  (algorithms/sgd_alg.py:48-59, compute_shifted_cosine_sim, as used by UProtoMF / IProtoMF / UIProtoMF, sgd_alg.py:380-399,
//            482-510) — sbr_proto_sim_*: the shifted similarity and the two arg-min regularisers behind it
//     e = W[rows[j], :]      sim[j, p] = clamp(1 + e^ . p^, 0, 2),  x^ = x / max(|x|, 1e-12)                       (F.normalize's eps)
//     proto_loss = mean_p min_j (2 - sim[j, p])          batch_loss = mean_j min_p (2 - sim[j, p])                  (sgd_alg.py:394-399)
//   ProtoMFs (sgd_alg.py:643-850: UProtoMFs / IProtoMFs / UIProtoMFs) — sbr_proto_score_*: the plain cosine (compute_cosine_sim,
//            sgd_alg.py:62-73) and, in the score form, the ReLU on the other entity's weights (sgd_alg.py:683, 739, 808, 814) and the
//            dot over the prototypes (sgd_alg.py:687, 750, 823-824) behind it; no regularisers, nothing takes a minimum
//     cos[j, p] = clamp(e^ . P^_p, -1, 1)      w[j, f, :] = Wt[widx[j fan + f], :]      out[j, f] = sum_p cos[j, p] max(w[j, f, p], 0)
//
// Arithmetic: fp32 FMA throughout. The raw dot products e . P[p] are accumulated first and divided by the product of the two clamped norms
// (max(|x|, eps), saved for the backward pass) afterwards; column and loss sums that cross workgroups are double. No float atomics.
//
// Tie rule (ProtoMF): a minimum attained more than once goes to the LOWEST index — the lowest prototype p for a row minimum, the lowest
// row j for a column minimum. The compared values are the fp32 distances 2 - sim themselves (the subtraction rounds for sim < 1, so two
// different similarities may tie as distances, as they do in the reference).
//
// Built on the 64 x 64 fp32 tile skeleton (csrc/tile64_f32.h; DESIGN.md has the work-item map, the LDS layout and the fixed-order rule).
// What crosses workgroups: ProtoMF's column minimum is taken per workgroup over its own rows (in LDS), written as one partial per
// workgroup, and picked over the partials in workgroup order by one workgroup; its row-minimum sum is one double per workgroup, added
// in workgroup order; dP (both ops) is written as one partial [P, D] per row split and folded in split order in double
// (t64_fold_kernel). The number of workgroups / splits depends on (R, D, P) only, never on the device. Unlike anchor_mix and
// cluster_affil this file keeps one 4 x 4 block per thread and walks the tiles:
//   forward   C[j, p] = sum_d e[j, d] P[p, d]      rows gathered straight from the table into LDS (the lookup is never materialised);
//                                                  the squared row norms are summed on the way in. P > 64: the prototype tiles are
//                                                  walked inside the row tile, the row tile comes back through the cache. This much
//                                                  is pc_cos_tile, once; the two forward kernels differ in what they do with cos.
//                                                  Score form: the clamped cosines of the tile go to LDS and every thread takes the
//                                                  outputs (j, f) = t, t + 256, ... of the tile: the weight row is read from the
//                                                  table, the ReLU applied in registers, four interleaved sums over p; out[j, f]
//                                                  takes the partial dots of the prototype tiles in tile order (the same thread owns
//                                                  an output in every tile).
//   dE        C[j, d] = sum_p g'[j, p] P^[p, d]    g' = the gradient into cos where the clamp passes (the closed interval, as torch.clamp)
//   dP        C[p, d] = sum_j g'[j, p] e^[j, d]    split over row ranges, partials folded in order
// followed by the projection terms of F.normalize's gradient ( - x^ (x^ . g) / |x| ), which need the row sums sum_p g' cos and the column
// sums sum_j g' cos: both are summed while g' is staged. The backward kernels live once; g' is a functor:
//   PsGrad       G - w_batch/R [p = argmin_p] - w_proto/P [j = argmin_j] on 0 <= 1 + cos <= 2               (sbr_proto_sim_bwd)
//   PqGivenGrad  a given G_cos [R, P] on -1 <= cos <= 1                                                     (sbr_proto_score_bwd, cosine form)
//   PqScoreGrad  sum_f g[j, f] max(w[j, f, p], 0) on -1 <= cos <= 1, the weight rows read again from the table      (..., score form)
// The weight-row gradient dWrows[j fan + f, p] = g[j, f] cos[j, p] [w > 0] is one element-wise pass.
//
// Saved by either forward for the backward: the un-clamped cosine [R, P], {max(|e|, eps), |e| >= eps} per row, the same per prototype
// (ProtoMF: and the two arg-mins). The gathered (and relu'd) weights are never written.
#include "tile64_f32.h"

namespace {

constexpr int PC_MAX_D = T64_MAX_D, PC_MAX_P = T64_MAX_N;
constexpr int PC_MAX_WG = 8192;     // dE and ProtoMFs forward workgroups: a grid-stride loop over the row tiles beyond it
constexpr int PS_MAX_WG = 256;      // ProtoMF forward workgroups = column-minimum partials
constexpr int PC_MAX_SPLIT = 256;   // dP row splits (times D tiles times P tiles workgroups)
constexpr int PQ_LDC = T64_T + 1;   // row stride of the cosine tile in LDS: a thread walks a row, neighbours hold other rows

inline bool pc_shape_ok(int D, int NP) { return D >= 1 && D <= PC_MAX_D && NP >= 2 && NP <= PC_MAX_P; }
static inline int ps_fwd_wgs(long R) { return t64_wgs(R, PS_MAX_WG); }
static inline int pc_splits(long R, int D, int NP) {
  int s = PC_MAX_SPLIT / (t64_tiles(D) * t64_tiles(NP));
  const int t = t64_tiles(R);
  if (s > t) s = t;
  return s < 1 ? 1 : s;
}

// ProtoMF's forward workspace: [wg doubles: row-minimum sums][2 * PC_MAX_P floats: prototype stats][wg * P floats][wg * P ints]
static inline size_t ps_fwd_ws_bytes(long R, int NP) {
  const size_t wg = (size_t)ps_fwd_wgs(R);
  return wg * sizeof(double) + 2 * PC_MAX_P * sizeof(float) + wg * NP * (sizeof(float) + sizeof(int));
}
// ProtoMFs' forward workspace: [2 * PC_MAX_P floats: prototype stats]
static inline size_t pq_fwd_ws_bytes() { return 2 * PC_MAX_P * sizeof(float); }
// backward workspace: [splits * P * D floats: dP partials][splits * P floats: column sums of g' cos]
static inline size_t pc_bwd_ws_bytes(long R, int D, int NP) { return (size_t)pc_splits(R, D, NP) * NP * ((size_t)D + 1) * sizeof(float); }

// (v, i) <- the smaller of (v, i) and (v2, i2); equal values: the lower index
__device__ __forceinline__ void ps_take_min(float& v, int& i, float v2, int i2) {
  if (v2 < v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
// torch.clamp(x, -1, 1) and torch.relu: a NaN stays a NaN
__device__ __forceinline__ float pq_clamp(float x) { return x < -1.f ? -1.f : (x > 1.f ? 1.f : x); }
__device__ __forceinline__ float pq_relu(float w) { return w <= 0.f ? 0.f : w; }

// ---- forward ---------------------------------------------------------------------------------------------------------------------------

// The front end of both forward kernels, for the row tile at j0 and the prototype tile pt: acc[i][c] <- the un-clamped cosine of row
// j0 + 4 rg + i and prototype 64 pt + 4 cg + c (exactly 0 in the padding). rp: the tile's row pointers (t64_row_ptrs), set by the caller
// once per row tile — setting them here, under pt == 0, costs every forward kernel an occupancy step. The first prototype tile of a row
// tile leaves the clamped row norms in s_rnc (and in row_stat, where given) for the later ones.
__device__ __forceinline__ void pc_cos_tile(float* __restrict__ As, float* __restrict__ Bs, float* __restrict__ s_rnc,
                                            const float* const (&rp)[8], long j0, long R, int D, const float* __restrict__ P, int pt, int NP,
                                            const float* __restrict__ pstat, float* __restrict__ row_stat, int t, float (&acc)[4][4]) {
  const int cg = t & 15, rg = t >> 4;
  const int sk = t & 31, sr = t >> 5;                 // staging of a transposed tile: k within the chunk, first of 8 rows (stride 8)
  float ss[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) ss[q] = 0.f;
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
    const float enc = s_rnc[4 * rg + i];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = acc[i][c] / (enc * pnc[c]);       // both factors >= 1e-12: the product is a normal number
  }
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
  __shared__ float s_colv[PC_MAX_P];
  __shared__ int s_colj[PC_MAX_P];
  __shared__ float s_wv[4][T64_T];
  __shared__ int s_wj[4][T64_T];
  __shared__ float s_rowdis[T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4, lane = t & 63, wave = t >> 6;
  if (STATS) {
    for (int p = t; p < PC_MAX_P; p += 256) { s_colv[p] = INFINITY; s_colj[p] = INT_MAX; }
  }
  double rowsum = 0.0;                                // thread 0: sum of this workgroup's row minima, in tile order
  const int n_pt = (NP + T64_T - 1) / T64_T;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    const float* rp[8];
    t64_row_ptrs(rp, W, ldw, rows, j0, R, t >> 5);        // sr = t >> 5, the staging row of pc_cos_tile
    float rbv[4];
    int rbp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { rbv[i] = INFINITY; rbp[i] = INT_MAX; }
    for (int pt = 0; pt < n_pt; ++pt) {
      float acc[4][4];
      pc_cos_tile(As, Bs, s_rnc, rp, j0, R, D, P, pt, NP, pstat, row_stat, t, acc);
      float cbv[4];
      int cbj[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) { cbv[c] = INFINITY; cbj[c] = INT_MAX; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long j = j0 + 4 * rg + i;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int p = pt * T64_T + 4 * cg + c;
          if (j < R && p < NP) {
            const float cs = acc[i][c];
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
  __shared__ float s_v[PC_MAX_P];
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
  const int n_pt = (NP + T64_T - 1) / T64_T;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    const float* rp[8];
    t64_row_ptrs(rp, W, ldw, rows, j0, R, t >> 5);        // sr = t >> 5, the staging row of pc_cos_tile
    for (int pt = 0; pt < n_pt; ++pt) {
      float acc[4][4];
      pc_cos_tile(As, Bs, s_rnc, rp, j0, R, D, P, pt, NP, pstat, row_stat, t, acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long j = j0 + 4 * rg + i;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int p = pt * T64_T + 4 * cg + c;
          float cc = 0.f;
          if (j < R && p < NP) {
            const float cs = acc[i][c];
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

// ---- backward: g'[j, p] = Grad::at(j, p, cs), with cs the un-clamped cosine it belongs to ------------------------------------------------------
// A functor is passed by value; prepare() runs once per thread before the first at().

// ProtoMF: G minus the arg-min shares of the two regularisers, on the closed interval where torch.clamp passes the gradient
struct PsGrad {
  const float* G;
  const float* g_proto;         // upstream gradients of the two regularisers: device scalars, NULL = 0
  const float* g_batch;
  const float* cos_raw;
  const int* row_best;
  const int* col_best_row;
  long R;
  int NP;
  float w_proto, w_batch;       // those gradients x 1 / P, x 1 / R (prepare)
  __device__ __forceinline__ void prepare() {
    w_proto = g_proto ? *g_proto / (float)NP : 0.f;
    w_batch = g_batch ? *g_batch / (float)R : 0.f;
  }
  __device__ __forceinline__ float at(long j, int p, float& cs) const {
    cs = cos_raw[j * NP + p];
    const float x = 1.f + cs;
    float g = G[j * NP + p];
    if (row_best[j] == p) g -= w_batch;
    if (col_best_row[p] == (int)j) g -= w_proto;
    return (x >= 0.f && x <= 2.f) ? g : 0.f;
  }
};
// ProtoMFs, cosine form: a given G_cos [R, P] ...
struct PqGivenGrad {
  const float* G;
  const float* cos_raw;
  int NP;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ float at(long j, int p, float& cs) const {
    cs = cos_raw[j * NP + p];
    const float g = G[j * NP + p];
    return (cs >= -1.f && cs <= 1.f) ? g : 0.f;
  }
};
// ... score form: sum_f g[j, f] max(w[j, f, p], 0), f ascending
struct PqScoreGrad {
  const float* g;
  const float* cos_raw;
  const float* Wt;
  const int* widx;
  long ldwt;
  int fan, NP;
  __device__ __forceinline__ void prepare() {}
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
__global__ __launch_bounds__(256) void pc_bwd_de_kernel(Grad gr, const float* __restrict__ W, long ldw, const int* __restrict__ rows, long R,
                                                        int D, const float* __restrict__ P, int NP, const float* __restrict__ row_stat,
                                                        const float* __restrict__ pstat, float* __restrict__ dE, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_S[T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int sk = t & 31, sr = t >> 5;                 // g' tile, transposed: prototype within the chunk, first of 8 rows
  const int bc = t & 63, bk = t >> 6;                 // prototype tile, as stored: column, first of 8 k (stride 4)
  gr.prepare();
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
__global__ __launch_bounds__(256) void pc_bwd_dp_kernel(Grad gr, const float* __restrict__ W, long ldw, const int* __restrict__ rows, long R,
                                                        int D, int NP, const float* __restrict__ row_stat, float* __restrict__ part,
                                                        float* __restrict__ part_t, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_T[4][T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int bc = t & 63, bk = t >> 6;                 // both operands as stored: column, first of 8 k (stride 4)
  gr.prepare();
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
struct PcFoldEpi {
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

// What the two backward entry points (`who`) share behind their own operand checks: dE, then dP as the ordered fold of its row splits.
// R = 0 zeroes dP.
template <class Grad>
int pc_bwd(const char* who, const Grad& gr, const float* W, long ldw, const int* rows, long R, int D, const float* P, int n_proto,
           const float* row_stat, const float* proto_stat, float* dE, float* dP, void* workspace, long workspace_bytes, hipStream_t s) {
  if (R == 0) {
    if (dP) {
      hipError_t e = hipMemsetAsync(dP, 0, (size_t)n_proto * D * sizeof(float), s);
      SBR_REQUIRE(e == hipSuccess, "%s: memset failed: %s", who, hipGetErrorString(e));
    }
    return SBR_OK;
  }
  const int n_tiles = t64_tiles(R);
  if (dE)
    pc_bwd_de_kernel<<<t64_wgs(R, PC_MAX_WG), 256, 0, s>>>(gr, W, ldw, rows, R, D, P, n_proto, row_stat, proto_stat, dE, n_tiles);
  if (dP) {
    SBR_REQUIRE(workspace && workspace_bytes >= (long)pc_bwd_ws_bytes(R, D, n_proto), "%s: workspace of %ld bytes, needs %ld", who,
                workspace_bytes, (long)pc_bwd_ws_bytes(R, D, n_proto));
    const int n_split = pc_splits(R, D, n_proto);
    float* part = (float*)workspace;
    float* part_t = part + (size_t)n_split * n_proto * D;
    const dim3 grid(n_split, t64_tiles(D), t64_tiles(n_proto));
    pc_bwd_dp_kernel<<<grid, 256, 0, s>>>(gr, W, ldw, rows, R, D, n_proto, row_stat, part, part_t, n_tiles);
    t64_fold_kernel<<<sbr_cdiv((long)n_proto * D, 256), 256, 0, s>>>(part, part_t, n_split, n_proto, D, PcFoldEpi{P, proto_stat}, dP);
  }
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}

}  // namespace

// ---- ProtoMF ---------------------------------------------------------------------------------------------------------------------------

extern "C" long sbr_proto_sim_workspace(long R, int D, int n_proto, int backward) {
  if (R <= 0 || !pc_shape_ok(D, n_proto)) return 0;
  return (long)(backward ? pc_bwd_ws_bytes(R, D, n_proto) : ps_fwd_ws_bytes(R, n_proto));
}

extern "C" int sbr_proto_sim_fwd(const float* W, long ldw, const int* rows, long R, int D, const float* P, int n_proto, float* sim_out,
                                 float* cos_raw, float* row_stat, float* proto_stat, int* row_best, float* col_best_val,
                                 int* col_best_row, float* proto_loss, float* batch_loss, void* workspace, long workspace_bytes,
                                 void* stream) {
  SBR_REQUIRE(pc_shape_ok(D, n_proto), "sbr_proto_sim_fwd: needs 1 <= D <= %d and 2 <= n_proto <= %d (got D = %d, n_proto = %d)", PC_MAX_D,
              PC_MAX_P, D, n_proto);
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
  float* part_cv = pstat + 2 * PC_MAX_P;
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
  SBR_REQUIRE(pc_shape_ok(D, n_proto), "sbr_proto_sim_bwd: needs 1 <= D <= %d and 2 <= n_proto <= %d (got D = %d, n_proto = %d)", PC_MAX_D,
              PC_MAX_P, D, n_proto);
  if (R != 0) {
    SBR_REQUIRE(R > 0 && R < INT_MAX && ldw >= D, "sbr_proto_sim_bwd: needs 0 <= R < 2^31 and ldw >= D");
    SBR_REQUIRE(G && W && P && cos_raw && row_stat && proto_stat && row_best && col_best_row, "sbr_proto_sim_bwd: null operand");
  }
  const PsGrad gr{G, g_proto, g_batch, cos_raw, row_best, col_best_row, R, n_proto, 0.f, 0.f};
  return pc_bwd("sbr_proto_sim_bwd", gr, W, ldw, rows, R, D, P, n_proto, row_stat, proto_stat, dE, dP, workspace, workspace_bytes,
                (hipStream_t)stream);
}

// ---- ProtoMFs --------------------------------------------------------------------------------------------------------------------------

extern "C" long sbr_proto_score_workspace(long R, int D, int n_proto, int backward) {
  if (R <= 0 || !pc_shape_ok(D, n_proto)) return 0;
  return (long)(backward ? pc_bwd_ws_bytes(R, D, n_proto) : pq_fwd_ws_bytes());
}

#define PQ_REQUIRE_SHAPE(who)                                                                                                          \
  SBR_REQUIRE(pc_shape_ok(D, n_proto) && fan >= 1, who ": needs 1 <= D <= %d, 2 <= n_proto <= %d and 1 <= fan (got D = %d, n_proto = %d, " \
              "fan = %d)", PC_MAX_D, PC_MAX_P, D, n_proto, fan)

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
  const int n_tiles = t64_tiles(R), nb = t64_wgs(R, PC_MAX_WG);
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
  if (R != 0) {
    SBR_REQUIRE(R > 0 && R < INT_MAX && R * (long)fan < INT_MAX && ldw >= D,
                "sbr_proto_score_bwd: needs 0 <= R, R * fan < 2^31 and ldw >= D (got R = %ld, fan = %d)", R, fan);
    SBR_REQUIRE(G && W && P && cos_raw && row_stat && proto_stat, "sbr_proto_score_bwd: null operand");
    SBR_REQUIRE(Wt ? ldwt >= n_proto : (!dWrows && !widx),
                "sbr_proto_score_bwd: the score form needs Wt and ldwt >= n_proto; the cosine form has neither dWrows nor widx");
    if (dWrows) {
      const long n = R * (long)fan * n_proto;
      const long blocks = sbr_cdiv(n, 256);
      pq_bwd_dw_kernel<<<(int)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>(G, cos_raw, Wt, ldwt, widx, fan, n_proto, n, dWrows);
    }
  }
  const char* who = "sbr_proto_score_bwd";
  if (Wt)
    return pc_bwd(who, PqScoreGrad{G, cos_raw, Wt, widx, ldwt, fan, n_proto}, W, ldw, rows, R, D, P, n_proto, row_stat, proto_stat, dE, dP,
                  workspace, workspace_bytes, s);
  return pc_bwd(who, PqGivenGrad{G, cos_raw, n_proto}, W, ldw, rows, R, D, P, n_proto, row_stat, proto_stat, dE, dP, workspace,
                workspace_bytes, s);
}
