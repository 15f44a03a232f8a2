// ACF's anchor mixing (algorithms/sgd_alg.py:261-276: get_user_representations / get_item_representations of ACF, Barkan et al., CIKM
// 2021) with the embedding lookup in front of it and the two entropy regularisers of ACF.forward (sgd_alg.py:246-254) behind it, forward
// and backward:
//     e = W[rows[j], :]     s = e . A^T     c = softmax(s)     r = c . A                        lse[j] = logsumexp_k s[j, k]
//     exc = mean_j H_j,  H_j = - sum_k c[j, k] (s[j, k] - lse[j])                               (entropy_from_softmax, sgd_alg.py:76-85)
//     inc = log K + sum_k q_k log q_k,  q_k = sum_j c[j, k] / sum_jk c[j, k]                     (sgd_alg.py:251-254)
//
// Arithmetic: fp32 FMA throughout, the softmax max-subtracted (p = exp(s - max), c = p / sum p); sums that cross workgroups are double.
// log c is never taken: the entropy and its gradient use s - lse, which is finite where c has underflowed to an exact 0 (5 % of the
// entries at D = 512, K = 256 with N(0, 1) operands), so the backward pass recomputes s instead of reading a logits matrix.
//
// NaN contract (the reference's): a column of c that is 0 in every row gives q_k == 0 and inc = NaN (0 log 0), and so are the gradients
// that flow through inc. Nothing is clamped. r, c, lse and exc do not depend on q and stay finite.
//
// Built on the 64 x 64 fp32 tile skeleton (csrc/tile64_f32.h; DESIGN.md has the work-item map, the LDS layout and the fixed-order rule):
// a workgroup keeps its tile of 64 rows for every product that shares the rows, and a thread holds a 4 x 4 block of every 64-wide anchor
// tile of the [64, K] logits in registers (K <= 256: up to four blocks, the template parameter), so the softmax, the entropies and the
// softmax backward are register arithmetic plus shuffles over the 16 lanes of a row group. What crosses workgroups here, one form that is
// valid in deterministic mode: the column sums of c are kept per workgroup (double, in LDS, the workgroup's tiles in order), written as
// one partial per workgroup and folded in workgroup order by one workgroup; the entropy sum is one double per workgroup, added in
// workgroup order; dA is one partial [K, D] per workgroup (= row split), folded in split order. The number of workgroups / splits depends
// on (R, D, K) only, never on the device.
//   forward   s = e A^T        the rows go from the table into LDS once (the lookup is never materialised), one staging of the row chunk
//                              serves every anchor tile
//             r = c A          c staged from the registers, per 64-wide tile of D
//   backward  dc = G A^T, s = e A^T (the loss form only) share the staged anchor chunk
//             ds = c (dc + g_inc log q_k / T - sum_m c_m dc_m) - g_exc / R c (s - lse + H)      (the gradient through the denominator T and
//                                                                                               the other per-row constants of dc vanish in
//                                                                                               the softmax backward)
//             dE = ds A        ds staged from the registers
//             dA = ds^T e + c^T G   one product over the 128 "rows" [ds; c] x [e; G] per (anchor tile, D tile), added into the partial
#include "tile64_f32.h"

namespace {

constexpr int AM_MAX_D = T64_MAX_D, AM_MAX_K = T64_MAX_N;
constexpr int AM_MAX_WG = T64_MAX_WG;      // workgroups of either pass = column-sum partials = dA row splits

static inline int am_fwd_wgs(long R) { return t64_wgs(R, AM_MAX_WG); }
static inline int am_splits(long R, int D, int K) { return t64_splits(R, (long)D * K); }
// forward workspace: [wg doubles: entropy sums][wg * K doubles: column sums of c]
static inline size_t am_fwd_ws_bytes(long R, int K) { return (size_t)am_fwd_wgs(R) * ((size_t)K + 1) * sizeof(double); }
// backward workspace: [splits * K * D floats: dA partials]
static inline size_t am_bwd_ws_bytes(long R, int D, int K) { return (size_t)am_splits(R, D, K) * K * D * sizeof(float); }

// out[j0 + row, :] = sum_k v[row, k] A[k, :]: v is the thread-held [64, K] block set (zero for k >= K)
template <int NPT>
__device__ __forceinline__ void am_times_anchors(float* __restrict__ As, float* __restrict__ Bs, const float (&v)[NPT][4][4],
                                                 const float* __restrict__ A, int K, int D, long j0, long R, float* __restrict__ out,
                                                 int t) {
  const int n_dt = (D + T64_T - 1) / T64_T;
  for (int dt = 0; dt < n_dt; ++dt) {
    float acc[4][4];
    t64_regs_times<NPT>(As, Bs, v, A, K, D, dt, t, acc);
    t64_store_rows(out, D, acc, j0, R, dt, D, t);
  }
}

template <int NPT, bool LOSS>
__global__ __launch_bounds__(256) void am_fwd_kernel(const float* __restrict__ W, long ldw, const int* __restrict__ rows, long R, int D,
                                                     const float* __restrict__ A, int K, float* __restrict__ r_out,
                                                     float* __restrict__ c_out, float* __restrict__ lse_out, double* __restrict__ part_cs,
                                                     double* __restrict__ part_h, int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ double s_col[AM_MAX_K];
  __shared__ float s_wc[4][T64_T];
  __shared__ float s_h[T64_T];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4, lane = t & 63, wave = t >> 6;
  const int sk = t & 31, sr = t >> 5;                 // staging of a transposed tile: k within the chunk, first of 8 rows (stride 8)
  if (LOSS) {
    s_col[t] = 0.0;                                   // 256 threads, AM_MAX_K entries; read after the barriers of the first tile
  }
  double hsum = 0.0;                                  // thread 0: sum of this workgroup's row entropies, in tile order
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    const float* rp[8];
    t64_row_ptrs(rp, W, ldw, rows, j0, R, sr);
    float v[NPT][4][4];                               // s, then c
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) t64_zero(v[pt]);
    for (int d0 = 0; d0 < D; d0 += T64_KC) {
      t64_stage_rows_t(As, rp, d0 + sk, D, sk, sr);
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        t64_stage_tile_t(Bs, A, pt, K, d0 + sk, D, sk, sr);
        __syncthreads();
        t64_mma(As, Bs, rg, cg, v[pt]);
        __syncthreads();
      }
    }
    // softmax of the four rows of this thread, entropy, outputs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long j = j0 + 4 * rg + i;
      float m = -INFINITY;
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (pt * T64_T + 4 * cg + c < K) m = fmaxf(m, v[pt][i][c]);
      m = t64_row_max(m);
      float sum = 0.f;
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (pt * T64_T + 4 * cg + c < K) sum += expf(v[pt][i][c] - m);
      sum = t64_row_sum(sum);
      const float lse = m + logf(sum);
      float h = 0.f;
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = pt * T64_T + 4 * cg + c;
          float cv = 0.f;
          if (k < K) {
            const float s = v[pt][i][c];
            cv = expf(s - m) / sum;
            h = fmaf(cv, s - lse, h);
            if (c_out && j < R) c_out[j * K + k] = cv;
          }
          v[pt][i][c] = cv;
        }
      if (LOSS) {
        h = t64_row_sum(h);
        if (cg == 0) s_h[4 * rg + i] = j < R ? -h : 0.f;
      }
      if (lse_out && cg == 0 && j < R) lse_out[j] = lse;
    }
    if (LOSS) {
      // column sums of c over the rows of this tile
      t64_col_sums<NPT>(s_wc, s_col, K, t, [&](int pt, int c) {
        float cs = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) cs += (j0 + 4 * rg + i < R) ? v[pt][i][c] : 0.f;
        return cs;
      });
      if (wave == 0) {
        const double hv = sbr_wave_sum_d((double)s_h[lane]);
        if (t == 0) hsum += hv;
      }
    }
    if (r_out) am_times_anchors<NPT>(As, Bs, v, A, K, D, j0, R, r_out, t);
    __syncthreads();                                  // s_h and the staging buffers belong to the next tile from here
  }
  if (LOSS) {
    for (int k = t; k < K; k += 256) part_cs[(long)blockIdx.x * K + k] = s_col[k];
    if (t == 0) part_h[blockIdx.x] = hsum;
  }
}

// the ordered fold of the workgroups' column sums and entropy sums, q, the saved d inc / d c and the two losses (one workgroup)
__global__ __launch_bounds__(256) void am_fin_kernel(const double* __restrict__ part_cs, const double* __restrict__ part_h, int nb, int K,
                                                     long R, float* __restrict__ q_out, float* __restrict__ dinc_out,
                                                     float* __restrict__ exc_loss, float* __restrict__ inc_loss) {
  __shared__ double s_S[AM_MAX_K];
  __shared__ double s_T;
  const int t = threadIdx.x;
  double S = 0.0;
  if (t < K) {
#pragma unroll 8
    for (int b = 0; b < nb; ++b) S += part_cs[(long)b * K + t];
    s_S[t] = S;
  }
  __syncthreads();
  if (t == 0) {
    double T = 0.0;
    for (int k = 0; k < K; ++k) T += s_S[k];
    s_T = T;
  }
  __syncthreads();
  const double T = s_T;
  if (t < K) {
    const double q = S / T, lq = log(q);
    q_out[t] = (float)q;
    dinc_out[t] = (float)(lq / T);
    s_S[t] = q * lq;                                  // q == 0: 0 * -inf = NaN, as in the reference
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += s_S[k];
    *inc_loss = (float)(log((double)K) + s);
  }
  if (t == 64) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part_h[b];
    *exc_loss = (float)(s / (double)R);
  }
}

template <int NPT, bool LOSS>
__global__ __launch_bounds__(256) void am_bwd_kernel(const float* __restrict__ G, const float* __restrict__ g_exc,
                                                     const float* __restrict__ g_inc, const float* __restrict__ W, long ldw,
                                                     const int* __restrict__ rows, long R, int D, const float* __restrict__ A, int K,
                                                     const float* __restrict__ c_in, const float* __restrict__ lse_in,
                                                     const float* __restrict__ dinc, float* __restrict__ dE, float* __restrict__ part,
                                                     int n_tiles) {
  __shared__ __align__(16) float As[T64_KC * T64_LD];
  __shared__ __align__(16) float Bs[T64_KC * T64_LD];
  __shared__ __align__(16) float Gs[T64_KC * T64_LD];
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
  const int sk = t & 31, sr = t >> 5;                 // transposed staging: k within the chunk, first of 8 rows (stride 8)
  const float w_exc = (LOSS && g_exc) ? *g_exc / (float)R : 0.f;
  const float w_inc = (LOSS && g_inc) ? *g_inc : 0.f;
  const int n_dt = (D + T64_T - 1) / T64_T;
  float* const my_part = part ? part + (long)blockIdx.x * K * D : nullptr;
  bool first = true;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long j0 = (long)tile * T64_T;
    const float* rp[8];
    const float* gp[8];
    t64_row_ptrs(rp, W, ldw, rows, j0, R, sr);
    t64_row_ptrs(gp, G, D, nullptr, j0, R, sr);
    float ds[NPT][4][4];                              // dc = G A^T, then ds
    float cv[NPT][4][4];                              // s = e A^T (the loss form), then c
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) { t64_zero(ds[pt]); t64_zero(cv[pt]); }
    for (int d0 = 0; d0 < D; d0 += T64_KC) {
      t64_stage_rows_t(Gs, gp, d0 + sk, D, sk, sr);
      if (LOSS) t64_stage_rows_t(As, rp, d0 + sk, D, sk, sr);
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        t64_stage_tile_t(Bs, A, pt, K, d0 + sk, D, sk, sr);
        __syncthreads();
        t64_mma(Gs, Bs, rg, cg, ds[pt]);
        if (LOSS) t64_mma(As, Bs, rg, cg, cv[pt]);
        __syncthreads();
      }
    }
    // softmax backward of the four rows of this thread, with the two regularisers' terms
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long j = j0 + 4 * rg + i;
      const float lse = (LOSS && j < R) ? lse_in[j] : 0.f;
      float dot = 0.f, h = 0.f;
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = pt * T64_T + 4 * cg + c;
          float cc = 0.f, l = 0.f, dc = 0.f;
          if (k < K && j < R) {
            cc = c_in[j * K + k];
            dc = ds[pt][i][c];
            if (LOSS) {
              l = cv[pt][i][c] - lse;                 // s - lse: finite where c is an exact 0
              if (w_inc != 0.f) dc = fmaf(w_inc, dinc[k], dc);
            }
          }
          dot = fmaf(cc, dc, dot);
          h = fmaf(cc, l, h);
          ds[pt][i][c] = dc;
          cv[pt][i][c] = LOSS ? l : cc;               // the loss form needs c, l and dc at once below: it reads c again (a cache hit)
        }
      dot = t64_row_sum(dot);
      h = LOSS ? t64_row_sum(h) : 0.f;                 // = -H_j
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = pt * T64_T + 4 * cg + c;
          float cc = 0.f, g = 0.f;
          if (k < K && j < R) {
            if (LOSS) {
              cc = c_in[j * K + k];
              g = cc * (ds[pt][i][c] - dot) - w_exc * (cc * (cv[pt][i][c] - h));
            } else {
              cc = cv[pt][i][c];
              g = cc * (ds[pt][i][c] - dot);
            }
          }
          ds[pt][i][c] = g;
          cv[pt][i][c] = cc;
        }
    }
    if (dE) am_times_anchors<NPT>(As, Bs, ds, A, K, D, j0, R, dE, t);
    if (my_part) {
      // dA[k, d] += sum_j ds[j, k] e[j, d] + sum_j c[j, k] G[j, d]: four chunks of 32 "rows" per output tile
      for (int dt = 0; dt < n_dt; ++dt) {
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
          float acc[4][4];
          t64_zero(acc);
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) {
            if (ch < 2) t64_regs_t_times(As, Bs, ds[pt], ch & 1, W, ldw, rows, j0, R, dt, D, t, acc);
            else t64_regs_t_times(As, Bs, cv[pt], ch & 1, G, D, nullptr, j0, R, dt, D, t, acc);
          }
          t64_part_add(my_part, acc, pt, K, dt, D, t, first);
        }
      }
    }
    first = false;
    __syncthreads();
  }
}

// dA[k, d] = the splits' partials added in split order (t64_fold_kernel)
struct AmFoldEpi {
  static constexpr bool kColumnSums = false;
  __device__ __forceinline__ float operator()(long, int, float s, float) const { return s; }
};

inline bool am_shape_ok(int D, int K) { return D >= 1 && D <= AM_MAX_D && K >= 2 && K <= AM_MAX_K; }

}  // namespace

extern "C" long sbr_anchor_mix_workspace(long R, int D, int n_anchors, int backward) {
  if (R <= 0 || !am_shape_ok(D, n_anchors)) return 0;
  return (long)(backward ? am_bwd_ws_bytes(R, D, n_anchors) : am_fwd_ws_bytes(R, n_anchors));
}

extern "C" int sbr_anchor_mix_fwd(const float* W, long ldw, const int* rows, long R, int D, const float* A, int n_anchors, float* r_out,
                                  float* c_out, float* lse_out, float* q_out, float* dinc_out, float* exc_loss, float* inc_loss,
                                  void* workspace, long workspace_bytes, void* stream) {
  const int K = n_anchors;
  SBR_REQUIRE(am_shape_ok(D, K), "sbr_anchor_mix_fwd: needs 1 <= D <= %d and 2 <= n_anchors <= %d (got D = %d, n_anchors = %d)", AM_MAX_D,
              AM_MAX_K, D, K);
  const bool loss = q_out || dinc_out || exc_loss || inc_loss;
  SBR_REQUIRE(!loss || (q_out && dinc_out && exc_loss && inc_loss),
              "sbr_anchor_mix_fwd: q, d inc / d c and the two losses come together (all or none)");
  if (R == 0) return SBR_OK;
  SBR_REQUIRE(R > 0 && R < INT_MAX && ldw >= D, "sbr_anchor_mix_fwd: needs 0 <= R < 2^31 and ldw >= D");
  SBR_REQUIRE(W && A && (r_out || c_out), "sbr_anchor_mix_fwd: null operand");
  SBR_REQUIRE(!loss || (workspace && workspace_bytes >= (long)am_fwd_ws_bytes(R, K)), "sbr_anchor_mix_fwd: workspace of %ld bytes, needs %ld",
              workspace_bytes, (long)am_fwd_ws_bytes(R, K));
  hipStream_t s = (hipStream_t)stream;
  const int nb = am_fwd_wgs(R), n_tiles = t64_tiles(R), npt = t64_tiles(K);
  if (loss) {
    double* part_h = (double*)workspace;
    double* part_cs = part_h + nb;
    t64_dispatch_npt(npt, [&](auto n) {
      am_fwd_kernel<decltype(n)::value, true><<<nb, 256, 0, s>>>(W, ldw, rows, R, D, A, K, r_out, c_out, lse_out, part_cs, part_h, n_tiles);
    });
    am_fin_kernel<<<1, 256, 0, s>>>(part_cs, part_h, nb, K, R, q_out, dinc_out, exc_loss, inc_loss);
  } else {
    t64_dispatch_npt(npt, [&](auto n) {
      am_fwd_kernel<decltype(n)::value, false><<<nb, 256, 0, s>>>(W, ldw, rows, R, D, A, K, r_out, c_out, lse_out, nullptr, nullptr, n_tiles);
    });
  }
  SBR_CHECK_LAUNCH("sbr_anchor_mix_fwd");
  return SBR_OK;
}

extern "C" int sbr_anchor_mix_bwd(const float* G, const float* g_exc, const float* g_inc, const float* W, long ldw, const int* rows,
                                  long R, int D, const float* A, int n_anchors, const float* c, const float* lse, const float* dinc,
                                  float* dE, float* dA, void* workspace, long workspace_bytes, void* stream) {
  const int K = n_anchors;
  SBR_REQUIRE(am_shape_ok(D, K), "sbr_anchor_mix_bwd: needs 1 <= D <= %d and 2 <= n_anchors <= %d (got D = %d, n_anchors = %d)", AM_MAX_D,
              AM_MAX_K, D, K);
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {
    if (dA) {
      hipError_t e = hipMemsetAsync(dA, 0, (size_t)K * D * sizeof(float), s);
      SBR_REQUIRE(e == hipSuccess, "sbr_anchor_mix_bwd: memset failed: %s", hipGetErrorString(e));
    }
    return SBR_OK;
  }
  SBR_REQUIRE(R > 0 && R < INT_MAX && ldw >= D, "sbr_anchor_mix_bwd: needs 0 <= R < 2^31 and ldw >= D");
  const bool loss = g_exc || g_inc;
  SBR_REQUIRE(G && W && A && c && (!loss || lse) && (!g_inc || dinc), "sbr_anchor_mix_bwd: null operand");
  if (!dE && !dA) return SBR_OK;
  SBR_REQUIRE(!dA || (workspace && workspace_bytes >= (long)am_bwd_ws_bytes(R, D, K)), "sbr_anchor_mix_bwd: workspace of %ld bytes, needs %ld",
              workspace_bytes, (long)am_bwd_ws_bytes(R, D, K));
  const int n_tiles = t64_tiles(R), npt = t64_tiles(K), nb = am_splits(R, D, K);
  float* part = dA ? (float*)workspace : nullptr;
  t64_dispatch_npt(npt, [&](auto n) {
    constexpr int NPT = decltype(n)::value;
    if (loss) am_bwd_kernel<NPT, true><<<nb, 256, 0, s>>>(G, g_exc, g_inc, W, ldw, rows, R, D, A, K, c, lse, dinc, dE, part, n_tiles);
    else am_bwd_kernel<NPT, false><<<nb, 256, 0, s>>>(G, g_exc, g_inc, W, ldw, rows, R, D, A, K, c, lse, dinc, dE, part, n_tiles);
  });
  if (dA) t64_fold_kernel<<<sbr_cdiv((long)K * D, 256), 256, 0, s>>>(part, nullptr, nb, K, D, AmFoldEpi{}, dA);
  SBR_CHECK_LAUNCH("sbr_anchor_mix_bwd");
  return SBR_OK;
}
