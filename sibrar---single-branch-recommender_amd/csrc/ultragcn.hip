// UltraGCN (Mao et al., CIKM 2021): two embedding tables trained on a degree-weighted pointwise loss and an item-item constraint term.
//   sbr_cooc_weight_topk                 the k largest omega_ij = count_ij * row_scale[i] * col_scale[j] of every row of a binary CSR
//                                        matrix: counting, value and top-k selection of one row inside one workgroup (knn.hip's scheme,
//                                        shared through csr_walk.h and cooc_topk.h)
//   sbr_ultragcn_loss_fwd_bwd            the three loss parts, dL/dUb and the coefficient matrix dL/ds of a batch in one pass over the
//                                        item rows, read straight from the table
//   sbr_scatter_add_scaled_rows_sorted   dst[j] += grad * sum coef * src over the slots that name row j, walked in ascending slot position
// No float atomics anywhere: the counts are integers, every float has one owner and a fixed operation order, so all three give the same
// bits on every run and are valid in deterministic mode. include/sibrar_hip.h states the same orders; tests/ultragcn_ref.py restates them.
#include "common.h"
#include "csr_walk.h"
#include "cooc_topk.h"
#include "slot_rows.h"

// ---------------------------------------------------------------------------------------------------------------------------------------
// neighbour lists
// ---------------------------------------------------------------------------------------------------------------------------------------
#define CW_THREADS 1024
#define CW_WAVES (CW_THREADS / 64)
#define CW_K_MAX 64
#define CW_DIM_MAX (1 << 24)         // counts are converted to fp32 exactly

// One workgroup per row i, as knn_topk_kernel: count, value in place, select per tile; sort and write after the last tile. The value of
// a cell with count c > 0 is (float(c) * row_scale[i]) * col_scale[j], two rounded multiplications, nothing contracted; a value that
// is not > 0 (a scale of 0) is no candidate.
__global__ __launch_bounds__(CW_THREADS) void cooc_weight_topk_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                                       const long* __restrict__ t_indptr, const int* __restrict__ t_indices,
                                                                       int n, int r0, const float* __restrict__ row_scale,
                                                                       const float* __restrict__ col_scale, int include_self, int k, int kpad,
                                                                       int tw, int* __restrict__ nbr_idx, float* __restrict__ nbr_val,
                                                                       int* __restrict__ nbr_len) {
#pragma clang fp contract(off)
  extern __shared__ unsigned int cnt[];
  __shared__ SbrTopkLds<CW_K_MAX> sel;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i = r0 + (int)blockIdx.x;
  const long f_beg = indptr[i], f_end = indptr[i + 1];
  const float rs = row_scale[i];
  int cur = 0;
  unsigned int n_list = 0;
  for (int t0 = 0; t0 < n && f_end > f_beg; t0 += tw) {
    const int t1 = t0 + tw < n ? t0 + tw : n, width = t1 - t0;
    for (int x = t; x < width; x += CW_THREADS) cnt[x] = 0u;
    __syncthreads();
    sbr_cooc_count_tile(indices, f_beg, f_end, t_indptr, t_indices, t0, width, w, CW_WAVES, lane, cnt);
    __syncthreads();
    for (int x = t; x < width; x += CW_THREADS) {
      const unsigned int c = cnt[x];
      const int j = t0 + x;
      if (c != 0u) {
        float v = (float)c * rs;
        v = v * col_scale[j];
        cnt[x] = (v > 0.f && (include_self || j != i)) ? __float_as_uint(v) : 0u;
      }
    }
    sbr_topk_select_tile<CW_THREADS>(sel, cnt, width, t0, k, cur, n_list);
  }
  sbr_topk_sort_write<CW_THREADS>(sel, cur, n_list, k, kpad, i, nbr_idx, nbr_val, nbr_len);
}

extern "C" int sbr_cooc_weight_topk(const long* indptr, const int* indices, const long* t_indptr, const int* t_indices, int n, int m, int r0,
                                    int r1, const float* row_scale, const float* col_scale, int include_self, int k, int tile_cols,
                                    int* nbr_idx, float* nbr_val, int* nbr_len, void* stream) {
  SBR_REQUIRE(k >= 1 && k <= CW_K_MAX, "sbr_cooc_weight_topk: k=%d outside [1, %d]", k, CW_K_MAX);
  SBR_REQUIRE(n >= 0 && m >= 0 && m <= CW_DIM_MAX, "sbr_cooc_weight_topk: shape [%d, %d] outside [0, 2^31) x [0, 2^24]", n, m);
  SBR_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= n, "sbr_cooc_weight_topk: row range [%d, %d) outside [0, %d]", r0, r1, n);
  const long fixed = (long)sizeof(SbrTopkLds<CW_K_MAX>) + 40;
  static SbrLdsSlot lds_slot;
  const int tw = sbr_row_tile("sbr_cooc_weight_topk", (const void*)cooc_weight_topk_kernel, &lds_slot, n, tile_cols, fixed, r1 - r0,
                              indptr && indices && t_indptr && t_indices && row_scale && col_scale && nbr_idx && nbr_val && nbr_len);
  if (tw <= 0) return -tw;
  int kpad = 2;
  while (kpad < k) kpad <<= 1;
  cooc_weight_topk_kernel<<<(unsigned)(r1 - r0), CW_THREADS, 4 * (size_t)tw, (hipStream_t)stream>>>(
      indptr, indices, t_indptr, t_indices, n, r0, row_scale, col_scale, include_self ? 1 : 0, k, kpad, tw, nbr_idx, nbr_val, nbr_len);
  SBR_CHECK_LAUNCH("sbr_cooc_weight_topk");
  return SBR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// the fused loss
// ---------------------------------------------------------------------------------------------------------------------------------------
#define UG_D_MAX 256
#define UG_K_MAX 64
#define UG_UNROLL 4                  // item rows in flight per lane group (the additions stay in slot order)

struct UgScalars {
  float w1, w2, w3, w4, neg_coef, lam;     // neg_coef = negative_weight / N, rounded once on the host side of the launch
};

// A batch row b belongs to a group of G = 2^gshift lanes, as a row of graph_prop.hip does: lane l of the group owns the V-wide chunks
// l, l + G, ... of the D columns (C of them), V = 4 when D % 4 == 0 and 1 otherwise, G the smallest power of two with G * V >= D up to
// a wave. A wave takes 64 / G consecutive batch rows; the workgroup is one wave. The group walks the row's 1 + N + K slots in ascending
// slot position: the positive, the N negatives, the K neighbour slots of the positive. It reads the slots' item index and weight G at
// a time, one per lane, hands them round by shuffles inside the group, and loads UG_UNROLL item rows before it uses the first.
// Per slot with a real item j:
//   s     = the lane's fmaf chain over its columns in ascending order from +0, then the xor butterfly over the group from offset G / 2
//           down to 1 (s = s + other): every lane of the group ends with the same bits
//   x     = -s at the positive and at a neighbour, s at a negative;  e = expf(-|x|)
//   sp    = max(x, 0) + log1pf(e);   sig = x >= 0 ? 1 / (1 + e) : e / (1 + e)
//   part += double(w * sp)           w: the slot's loss weight (header)
//   coef  = sgn * (cw * sig)         cw = w, neg_coef * w, lam * w;  sgn = -1, +1, -1
//   dUb  += coef * V[j]              one fmaf per owned column
// A padded neighbour slot (position >= len, or an index outside [0, n_items)) has coef +0 and reads no table row. Only the order of
// the loads is unrolled; every addition happens in slot order. The groups of a wave diverge only at padded slots; a shuffle's source
// lane is always in the reader's own group, which takes every branch together.
template <int V, int C>
__global__ __launch_bounds__(64) void ultragcn_loss_kernel(const float* __restrict__ Ub, const float* __restrict__ Vt,
                                                           const int* __restrict__ u_idxs, const int* __restrict__ i_idxs,
                                                           const float* __restrict__ beta_u, const float* __restrict__ beta_i,
                                                           const int* __restrict__ nbr_idx, const float* __restrict__ nbr_val,
                                                           const int* __restrict__ nbr_len, int B, int D, int N, int K, int n_users,
                                                           int n_items, UgScalars sc, int gshift, float* __restrict__ dUb,
                                                           float* __restrict__ coef, float* __restrict__ scores,
                                                           double* __restrict__ row_parts) {
#pragma clang fp contract(off)
  const int G = 1 << gshift;
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane - gl;
  const long b = ((long)blockIdx.x << (6 - gshift)) + (lane >> gshift);
  if (b >= B) return;
  const int n_slots = 1 + N + K;
  float ub[C][V], acc[C][V];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int col = (gl + k * G) * V;
#pragma unroll
    for (int j = 0; j < V; ++j) { ub[k][j] = 0.f; acc[k][j] = 0.f; }
    if (col < D) SbrRowChunk<V>::load(Ub + b * D + col, ub[k]);
  }
  const int u = u_idxs[b];
  const float bu = (unsigned int)u < (unsigned int)n_users ? beta_u[u] : 0.f;
  const int* my_items = i_idxs + b * (1 + N);
  const int p = my_items[0];
  const bool p_ok = (unsigned int)p < (unsigned int)n_items;
  int len = p_ok ? nbr_len[p] : 0;
  len = len < 0 ? 0 : (len > K ? K : len);
  double part[3] = {0., 0., 0.};
  for (int c0 = 0; c0 < n_slots; c0 += G) {
    const int n_e = n_slots - c0 < G ? n_slots - c0 : G;
    int my_j = -1;
    float my_w = 0.f;
    if (gl < n_e) {
      const int c = c0 + gl;
      if (c <= N) {
        my_j = my_items[c];
        if ((unsigned int)my_j < (unsigned int)n_items) {
          float t = bu * beta_i[my_j];
          t = (c == 0 ? sc.w2 : sc.w4) * t;
          my_w = (c == 0 ? sc.w1 : sc.w3) + t;
        }
      } else if (c - 1 - N < len) {
        my_j = nbr_idx[(long)p * K + (c - 1 - N)];
        my_w = nbr_val[(long)p * K + (c - 1 - N)];
      }
      if ((unsigned int)my_j >= (unsigned int)n_items) { my_j = -1; my_w = 0.f; }
    }
    for (int e0 = 0; e0 < n_e; e0 += UG_UNROLL) {
      float v[UG_UNROLL][C][V], wt[UG_UNROLL];
      int jj[UG_UNROLL];
#pragma unroll
      for (int q = 0; q < UG_UNROLL; ++q) {
        jj[q] = -1;
        if (e0 + q < n_e) {
          jj[q] = __shfl(my_j, gbase + e0 + q, 64);
          wt[q] = __shfl(my_w, gbase + e0 + q, 64);
          if (jj[q] >= 0) {
            const float* vr = Vt + (long)jj[q] * D;
#pragma unroll
            for (int k = 0; k < C; ++k) {
              const int col = (gl + k * G) * V;
              if (col < D) SbrRowChunk<V>::load(vr + col, v[q][k]);
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < UG_UNROLL; ++q) {
        if (e0 + q < n_e) {
          const int c = c0 + e0 + q;
          float cf = 0.f;
          if (jj[q] >= 0) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < C; ++k)
              if ((gl + k * G) * V < D) {
#pragma unroll
                for (int j = 0; j < V; ++j) s = fmaf(ub[k][j], v[q][k][j], s);
              }
            for (int off = G >> 1; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
            const int kind = c == 0 ? 0 : (c <= N ? 1 : 2);
            if (scores && kind != 2 && gl == 0) scores[b * (1 + N) + c] = s;
            const float sgn = kind == 1 ? 1.f : -1.f;
            const float x = sgn * s;
            const float e = expf(-fabsf(x));
            const float sp = fmaxf(x, 0.f) + log1pf(e);
            const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            part[kind] += (double)(wt[q] * sp);
            const float cw = kind == 0 ? wt[q] : (kind == 1 ? sc.neg_coef * wt[q] : sc.lam * wt[q]);
            cf = sgn * (cw * sig);
#pragma unroll
            for (int k = 0; k < C; ++k)
              if ((gl + k * G) * V < D) {
#pragma unroll
                for (int j = 0; j < V; ++j) acc[k][j] = fmaf(cf, v[q][k][j], acc[k][j]);
              }
          }
          if (gl == 0) {
            coef[b * n_slots + c] = cf;
            if (scores && c <= N && jj[q] < 0) scores[b * (1 + N) + c] = 0.f;     // an index outside the table: no score
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int col = (gl + k * G) * V;
    if (col < D) SbrRowChunk<V>::store(dUb + b * D + col, acc[k]);
  }
  if (gl == 0) {
    row_parts[3 * b] = part[0];
    row_parts[3 * b + 1] = part[1] / (double)N;
    row_parts[3 * b + 2] = part[2];
  }
}

// The fold of the per-row partials, in double: lane l of one wave adds the rows l, l + 64, ... in ascending order, then the xor
// butterfly from offset 32 down to 1. out = (pos, neg, nbr, pos + negative_weight * neg + lam * nbr), each rounded to fp32 once.
__global__ __launch_bounds__(64) void ultragcn_fold_kernel(const double* __restrict__ row_parts, int B, double negative_weight, double lam,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x;
  double s[3] = {0., 0., 0.};
  for (long b = lane; b < B; b += 64)
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += row_parts[3 * b + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = sbr_wave_sum_d(s[k]);
  if (lane == 0) {
    out[0] = (float)s[0];
    out[1] = (float)s[1];
    out[2] = (float)s[2];
    out[3] = (float)(s[0] + negative_weight * s[1] + lam * s[2]);
  }
}

template <int V, int C>
static void ug_launch(const float* Ub, const float* Vt, const int* u_idxs, const int* i_idxs, const float* beta_u, const float* beta_i,
                      const int* nbr_idx, const float* nbr_val, const int* nbr_len, int B, int D, int N, int K, int n_users, int n_items,
                      const UgScalars& sc, int gshift, float* dUb, float* coef, float* scores, double* row_parts, hipStream_t stream) {
  const long rows_per_block = 1L << (6 - gshift);
  ultragcn_loss_kernel<V, C><<<(unsigned)((B + rows_per_block - 1) / rows_per_block), 64, 0, stream>>>(
      Ub, Vt, u_idxs, i_idxs, beta_u, beta_i, nbr_idx, nbr_val, nbr_len, B, D, N, K, n_users, n_items, sc, gshift, dUb, coef, scores, row_parts);
}

extern "C" long sbr_ultragcn_loss_workspace(int B) { return B > 0 ? 24L * B : 0; }

extern "C" int sbr_ultragcn_loss_fwd_bwd(const float* Ub, const float* V, const int* u_idxs, const int* i_idxs, const float* beta_u,
                                         const float* beta_i, const int* nbr_idx, const float* nbr_val, const int* nbr_len, int B, int D,
                                         int N, int K, int n_users, int n_items, float w1, float w2, float w3, float w4,
                                         float negative_weight, float lam, float* parts, float* dUb, float* coef, float* scores,
                                         void* workspace, long workspace_bytes, void* stream) {
  const char* who = "sbr_ultragcn_loss_fwd_bwd";
  SBR_REQUIRE(D >= 1 && D <= UG_D_MAX, "%s: D=%d outside [1, %d]", who, D, UG_D_MAX);
  SBR_REQUIRE(N >= 1, "%s: N=%d: a batch row needs at least one negative", who, N);
  SBR_REQUIRE(K >= 1 && K <= UG_K_MAX, "%s: K=%d outside [1, %d]", who, K, UG_K_MAX);
  SBR_REQUIRE(B >= 0 && n_users >= 0 && n_items >= 0, "%s: negative shape (B=%d, n_users=%d, n_items=%d)", who, B, n_users, n_items);
  SBR_REQUIRE((long)B * (1L + N + K) <= 0x7FFFFFFFL, "%s: B (1 + N + K) = %ld slots, over 2^31 - 1", who, (long)B * (1L + N + K));
  SBR_REQUIRE(parts, "%s: null operand", who);
  SBR_REQUIRE(B == 0 || workspace_bytes >= sbr_ultragcn_loss_workspace(B), "%s: workspace of %ld bytes, %ld needed", who, workspace_bytes,
              sbr_ultragcn_loss_workspace(B));
  SBR_REQUIRE(B == 0 || (Ub && V && u_idxs && i_idxs && beta_u && beta_i && nbr_idx && nbr_val && nbr_len && dUb && coef && workspace),
              "%s: null operand", who);
  const SbrLaneGroup lg = sbr_lane_group(D);
  const bool vec = lg.vec;
  const int gshift = lg.gshift, per_lane = lg.per_lane;
  SBR_REQUIRE(!vec || ((uintptr_t)Ub | (uintptr_t)V | (uintptr_t)dUb) % 16 == 0, "%s: D=%d is read in 16-byte chunks: Ub, V and dUb must "
              "start on a 16-byte boundary", who, D);
  SBR_REQUIRE((uintptr_t)workspace % 8 == 0, "%s: the workspace must start on an 8-byte boundary", who);
  hipStream_t st = (hipStream_t)stream;
  if (B > 0) {
    UgScalars sc;
    sc.w1 = w1; sc.w2 = w2; sc.w3 = w3; sc.w4 = w4; sc.lam = lam;
    sc.neg_coef = negative_weight / (float)N;
#define UG_GO(VV, CC) ug_launch<VV, CC>(Ub, V, u_idxs, i_idxs, beta_u, beta_i, nbr_idx, nbr_val, nbr_len, B, D, N, K, n_users, n_items, sc, \
                                        gshift, dUb, coef, scores, (double*)workspace, st)
    if (vec) UG_GO(4, 1);                                         // D <= 256: at most 64 chunks, one per lane
    else if (per_lane <= 1) UG_GO(1, 1); else if (per_lane <= 2) UG_GO(1, 2); else UG_GO(1, 4);
#undef UG_GO
    SBR_CHECK_LAUNCH(who);
  }
  ultragcn_fold_kernel<<<1, 64, 0, st>>>((const double*)workspace, B, (double)negative_weight, (double)lam, parts);
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// the item-side gradient
// ---------------------------------------------------------------------------------------------------------------------------------------
// One wave per row j of dst. sorted_keys [n_slots] ascending: the wave finds its segment [lo, hi) by two binary searches (a row that no
// slot names is left alone; a key outside [0, n_rows) — the sentinel of a padded slot — is looked for by nobody). It reads the
// segment's slot positions order[q] 64 at a time, one per lane, and takes them in ascending q: lane l owns the columns l, l + 64, ...
// and adds acc = fmaf(coef[order[q]], src[order[q] / slots_per_row][col], acc) from +0; then dst[j][col] += grad[0] * acc (one rounded
// multiplication, one rounded addition). A position outside [0, n_slots) is skipped.
__global__ __launch_bounds__(64 * SBR_SORTED_WAVES) void scatter_scaled_sorted_kernel(const float* __restrict__ coef, const float* __restrict__ src,
                                                                              const int* __restrict__ sorted_keys,
                                                                              const long* __restrict__ order, long n_slots,
                                                                              int slots_per_row, const float* __restrict__ grad,
                                                                              float* __restrict__ dst, int n_rows, int D) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long j = (long)blockIdx.x * SBR_SORTED_WAVES + (threadIdx.x >> 6);
  if (j >= n_rows) return;
  long beg, end;
  sbr_sorted_segment(sorted_keys, n_slots, (int)j, beg, end);
  if (beg == end) return;
  float acc[SBR_SORTED_D_MAX / 64] = {0.f, 0.f, 0.f, 0.f}, unused = 0.f;
  sbr_sorted_row_walk<false>(coef, nullptr, src, order, beg, end, n_slots, slots_per_row, D, lane, acc, unused);
  const float g = grad[0];
#pragma unroll
  for (int k = 0; k < SBR_SORTED_D_MAX / 64; ++k) {
    const int col = lane + 64 * k;
    if (col < D) {
      const float t = g * acc[k];
      dst[j * D + col] = dst[j * D + col] + t;
    }
  }
}

extern "C" int sbr_scatter_add_scaled_rows_sorted(const float* coef, const float* src, const int* sorted_keys, const long* order, long n_slots,
                                                  int slots_per_row, const float* grad, float* dst, int n_rows, int D, void* stream) {
  const char* who = "sbr_scatter_add_scaled_rows_sorted";
  SBR_REQUIRE(D >= 1 && D <= SBR_SORTED_D_MAX, "%s: D=%d outside [1, %d]", who, D, SBR_SORTED_D_MAX);
  SBR_REQUIRE(n_slots >= 0 && n_slots <= 0x7FFFFFFFL && slots_per_row >= 1 && n_rows >= 0, "%s: bad shape (n_slots=%ld, slots_per_row=%d, "
              "n_rows=%d)", who, n_slots, slots_per_row, n_rows);
  SBR_REQUIRE(n_slots % slots_per_row == 0, "%s: %ld slots are no whole number of rows of %d", who, n_slots, slots_per_row);
  if (n_slots == 0 || n_rows == 0) return SBR_OK;
  SBR_REQUIRE(coef && src && sorted_keys && order && grad && dst, "%s: null operand", who);
  scatter_scaled_sorted_kernel<<<(unsigned)((n_rows + SBR_SORTED_WAVES - 1) / SBR_SORTED_WAVES), 64 * SBR_SORTED_WAVES, 0, (hipStream_t)stream>>>(
      coef, src, sorted_keys, order, n_slots, slots_per_row, grad, dst, n_rows, D);
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}
