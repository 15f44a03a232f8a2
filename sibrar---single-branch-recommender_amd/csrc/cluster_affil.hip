// ECF's sparse affiliation of a row to a small set of clusters (algorithms/sgd_alg.py:1020-1037, ECF._generate_item_representations, and
// sgd_alg.py:988-1009, ECF.get_user_representations; Du et al., WWW 2023), forward and backward, in two forms of one op:
//     cosine form (item side)   t[r, k] = clamp(W_r^ . Cl_k^, -1, 1),  x^ = x / max(|x|, 1e-12)      (compute_cosine_sim, sgd_alg.py:62-73)
//     logit form  (user side)   t[r, k] is an input
//     m[r, k]  = 1 at the `top` largest entries of row r, 0 elsewhere                                (topk + the index store)
//     p        = softmax(t / temp)           mh = p + (m - p)           x = sigmoid(t) * mh
// mh is formed in fp32 as the reference forms it: exactly 0 off the mask, fl(p + fl(1 - p)) on it. The mask carries no gradient (the
// reference detaches m - p), so with g = dL/dx
//     dt_k = g_k s'(t_k) mh_k + p_k (g_k s(t_k) - sum_j p_j g_j s(t_j)) / temp,      s = sigmoid, s' = s (1 - s)
// and the cosine form adds the upstream dL/dt (the user side's gradient into the item logits), passes the sum where the clamp was not
// active (torch.clamp: -1 <= raw <= 1) and continues through both normalisations into dW [R, D] (written directly: the rows ARE the
// table) and dCl [C, D]; a norm below eps takes torch's clamp_min gradient (no projection term).
//
// TIE RULE: equal logits at the mask boundary go to the LOWEST cluster index (-0 and +0 are equal). torch.topk leaves that order open.
//
// Top-k selection (exact, no sort): every logit is mapped to a 32-bit key whose unsigned order is the float order. The key of the
// `top`-th largest entry of a row is found by a radix search from the most significant bit down - 32 steps, each a count of "key >= the
// candidate" over the registers of the 16 lanes that hold the row, two rows' counts packed in one shuffle chain. Entries above that key
// are in the mask; of the entries equal to it, the first (top - number above) in index order are, by an exclusive prefix count over the
// 16 lanes (one byte per 64-wide cluster tile, packed in one word). No data-dependent loop: a row of equal values costs what any row costs.
//
// Saved for the backward pass (everything else is recomputed from t): row_state [R, 4] = {max_k t / temp, sum_k exp(t / temp - max),
// max(|W_r|, eps), |W_r| >= eps ? 1 : 0} (the last two in the cosine form only) and mask [R, ceil(C / 4)] bytes: bits 0 .. 3 of byte q =
// m of clusters 4 q .. 4 q + 3, bits 4 .. 7 = "the clamp was active" for the same clusters (a thread owns whole bytes: no cross-lane
// packing).
//
// Built on the 64 x 64 fp32 tile skeleton (csrc/tile64_f32.h; DESIGN.md has the work-item map, the LDS layout and the fixed-order rule):
// a thread holds a 4 x 4 block of every 64-wide cluster tile of the [64, C] logits in registers (C <= 256: up to four blocks, the
// template parameter), so selection, softmax and their backward are register arithmetic plus shuffles over the 16 lanes of a row group.
//   forward   raw = W Cl^T      rows go from the table into LDS once, their squared norms are summed on the way in; divided by the product of
//                               the two clamped norms afterwards
//   backward  dW  = (dt Cl^ - flag_r W^ (dt . t)) / |W_r|          dt staged from the registers, Cl^ = Cl / |Cl| staged per chunk
//             dCl = (dt^T W^ - flag_k Cl^ colsum_k(dt t)) / |Cl_k|
// What crosses workgroups here, one form that is valid in deterministic mode: dCl and the column sums of dt t are one partial per
// workgroup, folded in workgroup order in double. The number of workgroups depends on (R, D, C) only, never on the device. The forward
// pass has no cross-workgroup sum.
#include "tile64_f32.h"

namespace {

constexpr int CA_MAX_D = T64_MAX_D, CA_MAX_C = T64_MAX_N;
constexpr int CA_MAX_WG = T64_MAX_WG;      // workgroups of either pass = dCl partials

static inline int ca_fwd_wgs(long R) { return t64_wgs(R, CA_MAX_WG); }
static inline int ca_splits(long R, int D, int C) { return t64_splits(R, (long)(D + 1) * C); }
// workspace of either pass: [2 * CA_MAX_C floats: cluster stats {max(|Cl_k|, eps), |Cl_k| >= eps}], then, backward only,
// [splits * C * D floats: dCl partials][splits * C floats: column sums of dt t]
static inline size_t ca_fwd_ws_bytes() { return 2 * CA_MAX_C * sizeof(float); }
static inline size_t ca_bwd_ws_bytes(long R, int D, int C) {
  return ca_fwd_ws_bytes() + (size_t)ca_splits(R, D, C) * C * ((size_t)D + 1) * sizeof(float);
}

// t64_row_sum of counts
__device__ __forceinline__ unsigned ca_row_sum_u(unsigned v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// unsigned order of the keys == float order of the values; -0 and +0 share a key
__device__ __forceinline__ unsigned ca_key(float v) {
  const unsigned u = __float_as_uint(v + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float ca_sigmoid(float t) { return 1.f / (1.f + expf(-t)); }

// The exact top-`top` mask of the thread's four rows: mb[pt][i] bits 0 .. 3 = m of clusters 64 pt + 4 cg + (0 .. 3) of row i. Entries with
// k >= C never enter. All 16 lanes of a row group take every shuffle (rows past R hold zeros).
template <int NPT>
__device__ __forceinline__ void ca_select(const float (&v)[NPT][4][4], int C, int top, int cg, unsigned (&mb)[NPT][4]) {
  unsigned key[NPT][4][4];
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) key[pt][i][c] = (pt * T64_T + 4 * cg + c < C) ? ca_key(v[pt][i][c]) : 0u;   // candidates are >= 1
  unsigned pre[4] = {0u, 0u, 0u, 0u};
  const unsigned utop = (unsigned)top;
#pragma unroll 1
  for (int b = 31; b >= 0; --b) {
    const unsigned bit = 1u << b;
    unsigned c01 = 0u, c23 = 0u;                      // counts of rows (0, 1) and (2, 3), 16 bits each (<= 256)
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        c01 += (key[pt][0][c] >= (pre[0] | bit) ? 1u : 0u) + (key[pt][1][c] >= (pre[1] | bit) ? 0x10000u : 0u);
        c23 += (key[pt][2][c] >= (pre[2] | bit) ? 1u : 0u) + (key[pt][3][c] >= (pre[3] | bit) ? 0x10000u : 0u);
      }
    c01 = ca_row_sum_u(c01);
    c23 = ca_row_sum_u(c23);
    if ((c01 & 0xffffu) >= utop) pre[0] |= bit;
    if ((c01 >> 16) >= utop) pre[1] |= bit;
    if ((c23 & 0xffffu) >= utop) pre[2] |= bit;
    if ((c23 >> 16) >= utop) pre[3] |= bit;
  }
  // pre[i] = the key of the top-th largest entry: count(key > pre) < top <= count(key >= pre)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned n_gt = 0u, eq = 0u;                      // eq: one byte per cluster tile (<= 4 per lane, <= 64 per row group)
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        n_gt += key[pt][i][c] > pre[i] ? 1u : 0u;
        eq += key[pt][i][c] == pre[i] ? (1u << (8 * pt)) : 0u;
      }
    n_gt = ca_row_sum_u(n_gt);
    unsigned inc = eq;                                // inclusive prefix over the lanes of the row group, per byte
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const unsigned n = (unsigned)__shfl_up((int)inc, o, 16);
      if (cg >= o) inc += n;
    }
    const unsigned tot = (unsigned)__shfl((int)inc, 15, 16);
    const unsigned exc = inc - eq;
    const unsigned need = utop - n_gt;                // >= 1
    unsigned before_tiles = 0u;                       // equal entries in lower cluster tiles
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
      unsigned rank = before_tiles + ((exc >> (8 * pt)) & 0xffu);
      unsigned bits = 0u;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned k = key[pt][i][c];
        bool in = k > pre[i];
        if (k == pre[i]) { in = rank < need; ++rank; }
        if (in && pt * T64_T + 4 * cg + c < C) bits |= 1u << c;
      }
      mb[pt][i] = bits;
      before_tiles += (tot >> (8 * pt)) & 0xffu;
    }
  }
}

// Everything behind the logits of the thread's four rows: the mask, the softmax, mh and x; writes x, the row state and the mask bytes.
// v: t in. clampbits[pt][i]: bits 0 .. 3 "the clamp was active" (cosine form), 0 in the logit form.
template <int NPT>
__device__ __forceinline__ void ca_rows_fwd(const float (&v)[NPT][4][4], const unsigned (&clampbits)[NPT][4], int C, int top, float temp,
                                            long j0, long R, int rg, int cg, const float (&nr)[4], const float (&flag)[4],
                                            float* __restrict__ x_out, float* __restrict__ row_state, unsigned char* __restrict__ mask) {
  unsigned mb[NPT][4];
  ca_select<NPT>(v, C, top, cg, mb);
  const int C4 = (C + 3) >> 2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long j = j0 + 4 * rg + i;
    float m = -INFINITY;
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (pt * T64_T + 4 * cg + c < C) m = fmaxf(m, v[pt][i][c] / temp);
    m = t64_row_max(m);
    float sum = 0.f;
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (pt * T64_T + 4 * cg + c < C) sum += expf(v[pt][i][c] / temp - m);
    sum = t64_row_sum(sum);
    if (j < R) {
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = pt * T64_T + 4 * cg + c;
          if (k < C) {
            const float t = v[pt][i][c];
            const float p = expf(t / temp - m) / sum;
            const float mh = ((mb[pt][i] >> c) & 1u) ? p + (1.f - p) : 0.f;
            x_out[j * C + k] = ca_sigmoid(t) * mh;
          }
        }
        if (mask && pt * 16 + cg < C4) mask[j * C4 + pt * 16 + cg] = (unsigned char)(mb[pt][i] | (clampbits[pt][i] << 4));
      }
      if (row_state && cg == 0) *reinterpret_cast<float4*>(row_state + 4 * j) = make_float4(m, sum, nr[i], flag[i]);
    }
  }
}

// dt of the thread's four rows (zero for rows >= R and clusters >= C), rs[i] = sum_k dt t of row i (cosine form), tv = t
template <int NPT, bool COS>
__device__ __forceinline__ void ca_rows_bwd(float (&dt)[NPT][4][4], float (&tv)[NPT][4][4], float (&rs)[4], const float* __restrict__ G,
                                            const float* __restrict__ Gt, const float* __restrict__ T, int C, float temp, long j0, long R,
                                            int rg, int cg, const float* __restrict__ row_state, const unsigned char* __restrict__ mask) {
  const int C4 = (C + 3) >> 2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long j = j0 + 4 * rg + i;
    const bool live = j < R;
    const float m = live ? row_state[4 * j] : 0.f, sum = live ? row_state[4 * j + 1] : 1.f;
    float dot = 0.f;                                  // sum_k p_k g_k s_k
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = pt * T64_T + 4 * cg + c;
        float t = 0.f, g = 0.f;
        if (live && k < C) { t = T[j * C + k]; g = G[j * C + k]; dot = fmaf(expf(t / temp - m) / sum, g * ca_sigmoid(t), dot); }
        tv[pt][i][c] = t;
        dt[pt][i][c] = g;
      }
    dot = t64_row_sum(dot);
    float r = 0.f;
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
      const unsigned byte = (live && pt * 16 + cg < C4) ? mask[j * C4 + pt * 16 + cg] : 0u;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = pt * T64_T + 4 * cg + c;
        float d = 0.f;
        if (live && k < C) {
          const float t = tv[pt][i][c], g = dt[pt][i][c];
          const float s = ca_sigmoid(t), p = expf(t / temp - m) / sum;
          const float mh = ((byte >> c) & 1u) ? p + (1.f - p) : 0.f;
          d = g * (s * (1.f - s)) * mh + p * (g * s - dot) / temp;
          if (COS) {
            if (Gt) d += Gt[j * C + k];
            if ((byte >> (4 + c)) & 1u) d = 0.f;      // torch.clamp passes no gradient outside [-1, 1]
            r = fmaf(d, t, r);
          }
        }
        dt[pt][i][c] = d;
      }
    }
    rs[i] = COS ? t64_row_sum(r) : 0.f;
  }
}

template <int NPT>
__global__ __launch_bounds__(256) void ca_fwd_cos_kernel(const float* __restrict__ W, long ldw, long R, int D, const float* __restrict__ Cl,
                                                         int C, const float* __restrict__ cstat, int top, float temp,
                                                         float* __restrict__ t_out, float* __restrict__ x_out,
                                                         float* __restrict__ row_state, unsigned char* __restrict__ mask, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_ss[T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int sk = t & 31, sr = t >> 5;                 // staging of a transposed tile: k within the chunk, first of 8 rows (stride 8)
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    const float* rp[8];
    float ss[8];
    t64_row_ptrs(rp, W, ldw, nullptr, j0, R, sr);
#pragma unroll
    for (int q = 0; q < 8; ++q) ss[q] = 0.f;
    float v[NPT][4][4];                               // raw dot products, then t
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) t64_zero(v[pt]);
    for (int d0 = 0; d0 < D; d0 += T64_KC) {
      t64_stage_rows_t(As, rp, d0 + sk, D, sk, sr, ss, true);
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        t64_stage_tile_t(Bs, Cl, pt, C, d0 + sk, D, sk, sr);
        __syncthreads();
        t64_mma(As, Bs, rg, cg, v[pt]);
        __syncthreads();
      }
    }
    // squared row norms: the 32 lanes sk of a half wave hold the chunks' columns of rows sr + 8 q
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float s = t64_half_sum<false>(ss[q]);
      if (sk == 0) s_ss[sr + 8 * q] = s;
    }
    __syncthreads();
    float nr[4], flag[4];
    unsigned clampbits[NPT][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long j = j0 + 4 * rg + i;
      t64_stats(s_ss[4 * rg + i], nr[i], flag[i]);
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        unsigned cb = 0u;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = pt * T64_T + 4 * cg + c;
          float tv = 0.f;
          if (k < C) {
            const float raw = v[pt][i][c] / (nr[i] * cstat[2 * k]);
            if (raw < -1.f || raw > 1.f) cb |= 1u << c;
            tv = fminf(fmaxf(raw, -1.f), 1.f);
            if (t_out && j < R) t_out[j * C + k] = tv;
          }
          v[pt][i][c] = tv;
        }
        clampbits[pt][i] = cb;
      }
    }
    ca_rows_fwd<NPT>(v, clampbits, C, top, temp, j0, R, rg, cg, nr, flag, x_out, row_state, mask);
    __syncthreads();                                  // s_ss and the staging buffers belong to the next tile from here
  }
}

template <int NPT>
__global__ __launch_bounds__(256) void ca_fwd_logit_kernel(const float* __restrict__ T, long R, int C, int top, float temp,
                                                           float* __restrict__ x_out, float* __restrict__ row_state,
                                                           unsigned char* __restrict__ mask, int n_tiles) {
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    float v[NPT][4][4];
    unsigned clampbits[NPT][4];
    const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long j = j0 + 4 * rg + i;
        clampbits[pt][i] = 0u;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = pt * T64_T + 4 * cg + c;
          v[pt][i][c] = (j < R && k < C) ? T[j * C + k] : 0.f;
        }
      }
    ca_rows_fwd<NPT>(v, clampbits, C, top, temp, j0, R, rg, cg, zero4, zero4, x_out, row_state, mask);
  }
}

template <int NPT>
__global__ __launch_bounds__(256) void ca_bwd_logit_kernel(const float* __restrict__ G, const float* __restrict__ T, long R, int C, float temp,
                                                           const float* __restrict__ row_state, const unsigned char* __restrict__ mask,
                                                           float* __restrict__ dt_out, int n_tiles) {
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    float dt[NPT][4][4], tv[NPT][4][4], rs[4];
    ca_rows_bwd<NPT, false>(dt, tv, rs, G, nullptr, T, C, temp, j0, R, rg, cg, row_state, mask);
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long j = j0 + 4 * rg + i;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = pt * T64_T + 4 * cg + c;
          if (j < R && k < C) dt_out[j * C + k] = dt[pt][i][c];
        }
      }
  }
}

template <int NPT>
__global__ __launch_bounds__(256) void ca_bwd_cos_kernel(const float* __restrict__ G, const float* __restrict__ Gt, const float* __restrict__ W,
                                                         long ldw, long R, int D, const float* __restrict__ Cl, int C,
                                                         const float* __restrict__ cstat, const float* __restrict__ T, float temp,
                                                         const float* __restrict__ row_state, const unsigned char* __restrict__ mask,
                                                         float* __restrict__ dW, long lddw, float* __restrict__ part,
                                                         float* __restrict__ part_cs, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ float s_col[CA_MAX_C];
  __shared__ float s_wc[4][T64_T];
  // The two products below stage their operands here and not through t64_regs_times / t64_regs_t_times (anchor_mix.hip's): the same
  // statements behind a call cost this kernel a wave per SIMD at NPT = 1 and 16 bytes of scratch per lane at NPT = 4.
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int bc = t & 63, bk = t >> 6;                 // staging as stored: column, first of 8 k (stride 4)
  const int n_dt = (D + T64_T - 1) / T64_T;
  float* const my_part = part ? part + (long)blockIdx.x * C * D : nullptr;
  s_col[t] = 0.f;                                     // 256 threads, CA_MAX_C entries; read after the barriers of the first tile
  bool first = true;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    float dt[NPT][4][4], tv[NPT][4][4], rs[4];
    ca_rows_bwd<NPT, true>(dt, tv, rs, G, Gt, T, C, temp, j0, R, rg, cg, row_state, mask);
    if (my_part) {
      // column sums of dt t over the rows of this tile
      t64_col_sums<NPT>(s_wc, s_col, C, t, [&](int pt, int c) {
        float cs = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) cs = fmaf(dt[pt][i][c], tv[pt][i][c], cs);
        return cs;
      });
    }
    if (dW) {
      // dW[j, d] = (sum_k dt[j, k] Cl^[k, d] - flag_j W^[j, d] rs_j) / |W_j|
      float nr[4], flag[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long j = j0 + 4 * rg + i;
        nr[i] = j < R ? row_state[4 * j + 2] : 1.f;
        flag[i] = j < R ? row_state[4 * j + 3] : 0.f;
      }
      for (int dtile = 0; dtile < n_dt; ++dtile) {
        float acc[4][4];
        t64_zero(acc);
        const int d = dtile * T64_T + bc;
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int k0 = pt * T64_T + half * T64_KC;
            if (k0 < C) {                             // the same for every thread
              t64_stage_regs_t(As, dt[pt], half, rg, cg);
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                const int k = bk + 4 * q, kk = k0 + k;
                Bs[k * T64_LD + bc] = (kk < C && d < D) ? Cl[(long)kk * D + d] / cstat[2 * kk] : 0.f;
              }
              __syncthreads();
              t64_mma(As, Bs, rg, cg, acc);
              __syncthreads();
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long j = j0 + 4 * rg + i;
          if (j >= R) continue;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int dd = dtile * T64_T + 4 * cg + c;
            if (dd < D) dW[j * lddw + dd] = (acc[i][c] - flag[i] * (W[j * ldw + dd] / nr[i]) * rs[i]) / nr[i];
          }
        }
      }
    }
    if (my_part) {
      // partial of sum_j dt[j, k] W^[j, d]: two chunks of 32 rows per output tile
      for (int dtile = 0; dtile < n_dt; ++dtile) {
        const int d = dtile * T64_T + bc;
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
          float acc[4][4];
          t64_zero(acc);
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            t64_stage_regs(As, dt[pt], half, rg, cg);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const int rl = bk + 4 * q;
              const long j = j0 + half * T64_KC + rl;
              Bs[rl * T64_LD + bc] = (j < R && d < D) ? W[j * ldw + d] / row_state[4 * j + 2] : 0.f;
            }
            __syncthreads();
            t64_mma(As, Bs, rg, cg, acc);
            __syncthreads();
          }
          t64_part_add(my_part, acc, pt, C, dtile, D, t, first);
        }
      }
    }
    first = false;
    __syncthreads();
  }
  if (part_cs)
    for (int k = t; k < C; k += 256) part_cs[(long)blockIdx.x * C + k] = s_col[k];
}

// dCl[k, d] = (partials added in workgroup order - flag_k Cl^[k, d] (column sums added in workgroup order)) / |Cl_k| (t64_fold_kernel)
struct CaFoldEpi {
  static constexpr bool kColumnSums = true;
  const float* Cl;
  const float* cstat;
  __device__ __forceinline__ float operator()(long e, int k, float s, float cs) const {
    const float nc = cstat[2 * k], flag = cstat[2 * k + 1];
    return (s - flag * (Cl[e] / nc) * cs) / nc;
  }
};

inline bool ca_shape_ok(int C, int top, float temp) { return C >= 2 && C <= CA_MAX_C && top >= 1 && top <= C && temp > 0.f; }
inline bool ca_dim_ok(int D) { return D >= 1 && D <= CA_MAX_D; }

}  // namespace

extern "C" long sbr_cluster_affil_workspace(long R, int D, int n_clusters, int backward) {
  if (R <= 0 || !ca_dim_ok(D) || n_clusters < 2 || n_clusters > CA_MAX_C) return 0;
  return (long)(backward ? ca_bwd_ws_bytes(R, D, n_clusters) : ca_fwd_ws_bytes());
}

extern "C" int sbr_cluster_affil_fwd(const float* W, long ldw, const float* Cl, const float* t_in, long R, int D, int n_clusters, int top,
                                     float temp, float* t_out, float* x_out, float* row_state, unsigned char* mask, void* workspace,
                                     long workspace_bytes, void* stream) {
  const int C = n_clusters;
  const bool cosine = t_in == nullptr;
  SBR_REQUIRE(ca_shape_ok(C, top, temp), "sbr_cluster_affil_fwd: needs 2 <= n_clusters <= %d, 1 <= top <= n_clusters and temp > 0 (got "
              "n_clusters = %d, top = %d, temp = %g)", CA_MAX_C, C, top, (double)temp);
  if (R == 0) return SBR_OK;      // empty operands have no storage: their pointers may be NULL and do not name the form
  SBR_REQUIRE(!cosine || ca_dim_ok(D), "sbr_cluster_affil_fwd: needs 1 <= D <= %d (got D = %d)", CA_MAX_D, D);
  SBR_REQUIRE(cosine ? (W && Cl) : (!W && !Cl), "sbr_cluster_affil_fwd: the cosine form takes W and Cl, the logit form t_in alone");
  SBR_REQUIRE(R > 0 && R < INT_MAX && (!cosine || ldw >= D), "sbr_cluster_affil_fwd: needs 0 <= R < 2^31 and ldw >= D");
  SBR_REQUIRE(x_out, "sbr_cluster_affil_fwd: null operand");
  SBR_REQUIRE(!row_state || (((uintptr_t)row_state) & 15) == 0, "sbr_cluster_affil_fwd: row_state must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int nb = ca_fwd_wgs(R), n_tiles = t64_tiles(R), npt = t64_tiles(C);
  if (cosine) {
    SBR_REQUIRE(workspace && workspace_bytes >= (long)ca_fwd_ws_bytes(), "sbr_cluster_affil_fwd: workspace of %ld bytes, needs %ld",
                workspace_bytes, (long)ca_fwd_ws_bytes());
    float* cstat = (float*)workspace;
    t64_norm_kernel<<<sbr_cdiv(C, 4), 256, 0, s>>>(Cl, C, D, cstat, nullptr);
    t64_dispatch_npt(npt, [&](auto n) {
      ca_fwd_cos_kernel<decltype(n)::value><<<nb, 256, 0, s>>>(W, ldw, R, D, Cl, C, cstat, top, temp, t_out, x_out, row_state, mask, n_tiles);
    });
  } else {
    t64_dispatch_npt(npt, [&](auto n) {
      ca_fwd_logit_kernel<decltype(n)::value><<<nb, 256, 0, s>>>(t_in, R, C, top, temp, x_out, row_state, mask, n_tiles);
    });
  }
  SBR_CHECK_LAUNCH("sbr_cluster_affil_fwd");
  return SBR_OK;
}

extern "C" int sbr_cluster_affil_bwd(const float* G, const float* Gt, const float* W, long ldw, const float* Cl, const float* t, long R,
                                     int D, int n_clusters, float temp, const float* row_state, const unsigned char* mask, float* dW,
                                     long lddw, float* dCl, float* dt_out, void* workspace, long workspace_bytes, void* stream) {
  const int C = n_clusters;
  const bool cosine = W != nullptr || Cl != nullptr;
  SBR_REQUIRE(ca_shape_ok(C, 1, temp), "sbr_cluster_affil_bwd: needs 2 <= n_clusters <= %d and temp > 0 (got n_clusters = %d, temp = %g)",
              CA_MAX_C, C, (double)temp);
  SBR_REQUIRE(!cosine || ca_dim_ok(D), "sbr_cluster_affil_bwd: needs 1 <= D <= %d (got D = %d)", CA_MAX_D, D);
  // an empty table has no storage, so W may be NULL when R = 0
  SBR_REQUIRE(cosine ? ((W || R == 0) && Cl && !dt_out) : (!dW && !dCl && !Gt),
              "sbr_cluster_affil_bwd: the cosine form takes W and Cl and writes dW / dCl, the logit form writes dt_out");
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {
    if (dCl) {
      hipError_t e = hipMemsetAsync(dCl, 0, (size_t)C * D * sizeof(float), s);
      SBR_REQUIRE(e == hipSuccess, "sbr_cluster_affil_bwd: memset failed: %s", hipGetErrorString(e));
    }
    return SBR_OK;
  }
  SBR_REQUIRE(R > 0 && R < INT_MAX && (!cosine || (ldw >= D && (!dW || lddw >= D))),
              "sbr_cluster_affil_bwd: needs 0 <= R < 2^31, ldw >= D and lddw >= D");
  SBR_REQUIRE(G && t && row_state && mask, "sbr_cluster_affil_bwd: null operand");
  const int n_tiles = t64_tiles(R), npt = t64_tiles(C);
  if (!cosine) {
    if (!dt_out) return SBR_OK;
    const int nb = ca_fwd_wgs(R);
    t64_dispatch_npt(npt, [&](auto n) {
      ca_bwd_logit_kernel<decltype(n)::value><<<nb, 256, 0, s>>>(G, t, R, C, temp, row_state, mask, dt_out, n_tiles);
    });
    SBR_CHECK_LAUNCH("sbr_cluster_affil_bwd");
    return SBR_OK;
  }
  if (!dW && !dCl) return SBR_OK;
  SBR_REQUIRE(workspace && workspace_bytes >= (long)ca_bwd_ws_bytes(R, D, C), "sbr_cluster_affil_bwd: workspace of %ld bytes, needs %ld",
              workspace_bytes, (long)ca_bwd_ws_bytes(R, D, C));
  const int nb = ca_splits(R, D, C);
  float* cstat = (float*)workspace;
  float* part = dCl ? cstat + 2 * CA_MAX_C : nullptr;
  float* part_cs = dCl ? part + (long)nb * C * D : nullptr;
  t64_norm_kernel<<<sbr_cdiv(C, 4), 256, 0, s>>>(Cl, C, D, cstat, nullptr);
  t64_dispatch_npt(npt, [&](auto n) {
    ca_bwd_cos_kernel<decltype(n)::value><<<nb, 256, 0, s>>>(G, Gt, W, ldw, R, D, Cl, C, cstat, t, temp, row_state, mask, dW, lddw, part,
                                                             part_cs, n_tiles);
  });
  if (dCl) t64_fold_kernel<<<sbr_cdiv((long)C * D, 256), 256, 0, s>>>(part, part_cs, nb, C, D, CaFoldEpi{Cl, cstat}, dCl);
  SBR_CHECK_LAUNCH("sbr_cluster_affil_bwd");
  return SBR_OK;
}
