// SimpleX (Mao et al., CIKM 2021): the cosine contrastive loss (CCL) over one positive and N sampled negatives per batch row.
//   sbr_ccl_loss_fwd_bwd              the loss parts, dL/dH and the two coefficient arrays of the item-table gradient in one pass over the
//                                     item rows, read straight from the table; one read of a row gives <H[b], V[j]> and <V[j], V[j]>
//   sbr_scatter_add_cos_rows_sorted   dst[j] += grad * (sum coef_a * src + (sum coef_s) * V[j]) over the slots that name row j, walked in
//                                     ascending slot position (the walk of sbr_scatter_add_scaled_rows_sorted, csrc/slot_rows.h)
// No atomics: every float has one owner and a fixed operation order, so both give the same bits on every run and are valid in
// deterministic mode. include/sibrar_hip.h states the same orders; tests/simplex_ref.py restates them.
#include "common.h"
#include "slot_rows.h"

#define CCL_D_MAX 256
#define CCL_UNROLL 4                 // item rows in flight per lane group (the additions stay in slot order)

struct CclScalars {
  float margin, eps, g_pos, g_neg;   // g_pos = -fl(1 / B); g_neg = fl(fl(negative_weight / N) * fl(1 / B)), rounded on the host side
};

// A batch row b belongs to a group of G = 2^gshift lanes with the geometry of ultragcn_loss_kernel: lane l of the group owns the
// V-wide chunks l, l + G, ... of the D columns (C of them). A wave takes 64 / G consecutive batch rows; the workgroup is one wave.
// Every dot product below (hh, s, vv) is the lane's fmaf chain over its columns in ascending order from +0, then the xor butterfly over
// the group from offset G / 2 down to 1 (x = x + other): every lane of the group ends with the same bits.
//   hh = <H[b], H[b]>;  rh = sqrtf(hh);  nh = max(rh, eps)
// The group walks the 1 + N slots in ascending c, reads the item indices G at a time, one per lane, hands them round by shuffles and
// loads CCL_UNROLL item rows before it uses the first. Per slot with an index j inside the table:
//   s = <H[b], V[j]>;  vv = <V[j], V[j]>   from the same registers: one read of the row
//   rv = sqrtf(vv);  nv = max(rv, eps);  den = nh * nv;  y = s / den
//   c = 0:   term = 1 - y (to the positive part, in double);          g = g_pos
//   c >= 1:  term = max(y - margin, 0) (to the negative part);        g = y > margin ? g_neg : +0
//   g == 0:  coef_a = coef_s = +0, nothing more
//   else     coef_a = g / den;  gy = g * y;  sgy = sgy + gy;  coef_s = rv < eps ? +0 : -(gy / (nv * nv))
//            acc[d] = fmaf(coef_a, V[j][d], acc[d])   per owned column
// A slot whose index lies outside [0, n_items) reads no table row, scores 0, has both coefficients +0 and adds no term.
// After the last slot: k = rh < eps ? +0 : sgy / (nh * nh);  dH[b][d] = fmaf(-k, H[b][d], acc[d]).
// Only the order of the loads is unrolled. The groups of a wave diverge only at slots outside the table and at inactive negatives; a
// shuffle's source lane is always in the reader's own group, which takes every branch together (y and g are the same bits in the group).
template <int V, int C>
__global__ __launch_bounds__(64) void ccl_loss_kernel(const float* __restrict__ H, const float* __restrict__ Vt,
                                                      const int* __restrict__ i_idxs, int B, int D, int N, int n_items, CclScalars sc,
                                                      int gshift, float* __restrict__ dH, float* __restrict__ coef_a,
                                                      float* __restrict__ coef_s, float* __restrict__ scores,
                                                      double* __restrict__ row_parts) {
#pragma clang fp contract(off)
  const int G = 1 << gshift;
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane - gl;
  const long b = ((long)blockIdx.x << (6 - gshift)) + (lane >> gshift);
  if (b >= B) return;
  const int n_slots = 1 + N;
  float h[C][V], acc[C][V];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int col = (gl + k * G) * V;
#pragma unroll
    for (int j = 0; j < V; ++j) { h[k][j] = 0.f; acc[k][j] = 0.f; }
    if (col < D) SbrRowChunk<V>::load(H + b * D + col, h[k]);
  }
  float hh = 0.f;
#pragma unroll
  for (int k = 0; k < C; ++k)
    if ((gl + k * G) * V < D) {
#pragma unroll
      for (int j = 0; j < V; ++j) hh = fmaf(h[k][j], h[k][j], hh);
    }
  for (int off = G >> 1; off > 0; off >>= 1) hh = hh + __shfl_xor(hh, off, 64);
  const float rh = sqrtf(hh);
  const float nh = fmaxf(rh, sc.eps);
  const int* my_items = i_idxs + b * n_slots;
  double part[2] = {0., 0.};
  float sgy = 0.f;
  for (int c0 = 0; c0 < n_slots; c0 += G) {
    const int n_e = n_slots - c0 < G ? n_slots - c0 : G;
    int my_j = -1;
    if (gl < n_e) {
      my_j = my_items[c0 + gl];
      if ((unsigned int)my_j >= (unsigned int)n_items) my_j = -1;
    }
    for (int e0 = 0; e0 < n_e; e0 += CCL_UNROLL) {
      float v[CCL_UNROLL][C][V];
      int jj[CCL_UNROLL];
#pragma unroll
      for (int q = 0; q < CCL_UNROLL; ++q) {
        jj[q] = -1;
        if (e0 + q < n_e) {
          jj[q] = __shfl(my_j, gbase + e0 + q, 64);
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
      for (int q = 0; q < CCL_UNROLL; ++q) {
        if (e0 + q < n_e) {
          const int c = c0 + e0 + q;
          float ca = 0.f, cs = 0.f, y = 0.f;
          if (jj[q] >= 0) {
            float s = 0.f, vv = 0.f;
#pragma unroll
            for (int k = 0; k < C; ++k)
              if ((gl + k * G) * V < D) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                  s = fmaf(h[k][j], v[q][k][j], s);
                  vv = fmaf(v[q][k][j], v[q][k][j], vv);
                }
              }
            for (int off = G >> 1; off > 0; off >>= 1) {
              s = s + __shfl_xor(s, off, 64);
              vv = vv + __shfl_xor(vv, off, 64);
            }
            const float rv = sqrtf(vv);
            const float nv = fmaxf(rv, sc.eps);
            const float den = nh * nv;
            y = s / den;
            float g;
            if (c == 0) {
              part[0] += (double)(1.f - y);
              g = sc.g_pos;
            } else {
              part[1] += (double)fmaxf(y - sc.margin, 0.f);
              g = y > sc.margin ? sc.g_neg : 0.f;
            }
            if (g != 0.f) {
              ca = g / den;
              const float gy = g * y;
              sgy = sgy + gy;
              if (!(rv < sc.eps)) cs = -(gy / (nv * nv));
#pragma unroll
              for (int k = 0; k < C; ++k)
                if ((gl + k * G) * V < D) {
#pragma unroll
                  for (int j = 0; j < V; ++j) acc[k][j] = fmaf(ca, v[q][k][j], acc[k][j]);
                }
            }
          }
          if (gl == 0) {
            const long pos = b * n_slots + c;
            coef_a[pos] = ca;
            coef_s[pos] = cs;
            if (scores) scores[pos] = y;
          }
        }
      }
    }
  }
  const float k_self = rh < sc.eps ? 0.f : sgy / (nh * nh);
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int col = (gl + k * G) * V;
    if (col < D) {
#pragma unroll
      for (int j = 0; j < V; ++j) acc[k][j] = fmaf(-k_self, h[k][j], acc[k][j]);
      SbrRowChunk<V>::store(dH + b * D + col, acc[k]);
    }
  }
  if (gl == 0) {
    row_parts[2 * b] = part[0];
    row_parts[2 * b + 1] = part[1] / (double)N;
  }
}

// The fold of the per-row partials, in double: lane l of one wave adds the rows l, l + 64, ... in ascending order, then the xor
// butterfly from offset 32 down to 1. out = (pos / B, neg / B, (pos + negative_weight * neg) / B), each rounded to fp32 once.
__global__ __launch_bounds__(64) void ccl_fold_kernel(const double* __restrict__ row_parts, int B, double negative_weight,
                                                      float* __restrict__ out) {
  const int lane = threadIdx.x;
  double s[2] = {0., 0.};
  for (long b = lane; b < B; b += 64) {
    s[0] += row_parts[2 * b];
    s[1] += row_parts[2 * b + 1];
  }
  s[0] = sbr_wave_sum_d(s[0]);
  s[1] = sbr_wave_sum_d(s[1]);
  if (lane == 0) {
    const double n = B > 0 ? (double)B : 1.;
    out[0] = (float)(s[0] / n);
    out[1] = (float)(s[1] / n);
    out[2] = (float)((s[0] + negative_weight * s[1]) / n);
  }
}

template <int V, int C>
static void ccl_launch(const float* H, const float* Vt, const int* i_idxs, int B, int D, int N, int n_items, const CclScalars& sc, int gshift,
                       float* dH, float* coef_a, float* coef_s, float* scores, double* row_parts, hipStream_t stream) {
  const long rows_per_block = 1L << (6 - gshift);
  ccl_loss_kernel<V, C><<<(unsigned)((B + rows_per_block - 1) / rows_per_block), 64, 0, stream>>>(
      H, Vt, i_idxs, B, D, N, n_items, sc, gshift, dH, coef_a, coef_s, scores, row_parts);
}

extern "C" long sbr_ccl_loss_workspace(int B) { return B > 0 ? 16L * B : 0; }

extern "C" int sbr_ccl_loss_fwd_bwd(const float* H, const float* V, const int* i_idxs, int B, int D, int N, int n_items, float margin,
                                    float negative_weight, float eps, float* parts, float* dH, float* coef_a, float* coef_s, float* scores,
                                    void* workspace, long workspace_bytes, void* stream) {
  const char* who = "sbr_ccl_loss_fwd_bwd";
  SBR_REQUIRE(D >= 1 && D <= CCL_D_MAX, "%s: D=%d outside [1, %d]", who, D, CCL_D_MAX);
  SBR_REQUIRE(N >= 1, "%s: N=%d: a batch row needs at least one negative", who, N);
  SBR_REQUIRE(B >= 0 && n_items >= 0, "%s: negative shape (B=%d, n_items=%d)", who, B, n_items);
  SBR_REQUIRE((long)B * (1L + N) <= 0x7FFFFFFFL, "%s: B (1 + N) = %ld slots, over 2^31 - 1", who, (long)B * (1L + N));
  SBR_REQUIRE(eps > 0.f, "%s: eps=%g is not positive", who, (double)eps);
  SBR_REQUIRE(parts, "%s: null operand", who);
  SBR_REQUIRE(B == 0 || workspace_bytes >= sbr_ccl_loss_workspace(B), "%s: workspace of %ld bytes, %ld needed", who, workspace_bytes,
              sbr_ccl_loss_workspace(B));
  SBR_REQUIRE(B == 0 || (H && V && i_idxs && dH && coef_a && coef_s && workspace), "%s: null operand", who);
  const SbrLaneGroup lg = sbr_lane_group(D);
  SBR_REQUIRE(!lg.vec || ((uintptr_t)H | (uintptr_t)V | (uintptr_t)dH) % 16 == 0, "%s: D=%d is read in 16-byte chunks: H, V and dH must "
              "start on a 16-byte boundary", who, D);
  SBR_REQUIRE((uintptr_t)workspace % 8 == 0, "%s: the workspace must start on an 8-byte boundary", who);
  // the instantiations below hold 1 chunk per lane (4-wide chunks) and up to 4 (1-wide): a larger CCL_D_MAX needs more of them
  SBR_REQUIRE(lg.per_lane <= (lg.vec ? 1 : 4), "%s: D=%d needs %d chunks per lane, more than the kernel is built for", who, D, lg.per_lane);
  hipStream_t st = (hipStream_t)stream;
  if (B > 0) {
    CclScalars sc;
    const float inv_b = 1.f / (float)B, neg_coef = negative_weight / (float)N;
    sc.margin = margin; sc.eps = eps;
    sc.g_pos = -inv_b;
    sc.g_neg = neg_coef * inv_b;
#define CCL_GO(VV, CC) ccl_launch<VV, CC>(H, V, i_idxs, B, D, N, n_items, sc, lg.gshift, dH, coef_a, coef_s, scores, (double*)workspace, st)
    if (lg.vec) CCL_GO(4, 1);                                     // D <= 256: at most 64 chunks, one per lane
    else if (lg.per_lane <= 1) CCL_GO(1, 1); else if (lg.per_lane <= 2) CCL_GO(1, 2); else CCL_GO(1, 4);
#undef CCL_GO
    SBR_CHECK_LAUNCH(who);
  }
  ccl_fold_kernel<<<1, 64, 0, st>>>((const double*)workspace, B, (double)negative_weight, parts);
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// the item-side gradient
// ---------------------------------------------------------------------------------------------------------------------------------------
// One wave per row j of dst, the segment search and the walk of scatter_scaled_sorted_kernel (slot_rows.h): S[col] the fmaf chain of
// coef_a[pos] * src[pos / slots_per_row][col] and T the sum of coef_s[pos], both from +0 in ascending slot position. Then
//   r = fmaf(T, V[j][col], S[col]);  t = grad[0] * r;  dst[j][col] = dst[j][col] + t     one rounding each.
__global__ __launch_bounds__(64 * SBR_SORTED_WAVES) void scatter_cos_sorted_kernel(const float* __restrict__ coef_a, const float* __restrict__ coef_s,
                                                                           const float* __restrict__ src, const float* __restrict__ Vt,
                                                                           const int* __restrict__ sorted_keys,
                                                                           const long* __restrict__ order, long n_slots, int slots_per_row,
                                                                           const float* __restrict__ grad, float* __restrict__ dst,
                                                                           int n_rows, int D) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long j = (long)blockIdx.x * SBR_SORTED_WAVES + (threadIdx.x >> 6);
  if (j >= n_rows) return;
  long beg, end;
  sbr_sorted_segment(sorted_keys, n_slots, (int)j, beg, end);
  if (beg == end) return;
  float acc[SBR_SORTED_D_MAX / 64] = {0.f, 0.f, 0.f, 0.f}, tsum = 0.f;
  sbr_sorted_row_walk<true>(coef_a, coef_s, src, order, beg, end, n_slots, slots_per_row, D, lane, acc, tsum);
  const float g = grad[0];
#pragma unroll
  for (int k = 0; k < SBR_SORTED_D_MAX / 64; ++k) {
    const int col = lane + 64 * k;
    if (col < D) {
      const float r = fmaf(tsum, Vt[j * D + col], acc[k]);
      const float t = g * r;
      dst[j * D + col] = dst[j * D + col] + t;
    }
  }
}

extern "C" int sbr_scatter_add_cos_rows_sorted(const float* coef_a, const float* coef_s, const float* src, const float* V,
                                               const int* sorted_keys, const long* order, long n_slots, int slots_per_row, const float* grad,
                                               float* dst, int n_rows, int D, void* stream) {
  const char* who = "sbr_scatter_add_cos_rows_sorted";
  SBR_REQUIRE(D >= 1 && D <= SBR_SORTED_D_MAX, "%s: D=%d outside [1, %d]", who, D, SBR_SORTED_D_MAX);
  SBR_REQUIRE(n_slots >= 0 && n_slots <= 0x7FFFFFFFL && slots_per_row >= 1 && n_rows >= 0, "%s: bad shape (n_slots=%ld, slots_per_row=%d, "
              "n_rows=%d)", who, n_slots, slots_per_row, n_rows);
  SBR_REQUIRE(n_slots % slots_per_row == 0, "%s: %ld slots are no whole number of rows of %d", who, n_slots, slots_per_row);
  if (n_slots == 0 || n_rows == 0) return SBR_OK;
  SBR_REQUIRE(coef_a && coef_s && src && V && sorted_keys && order && grad && dst, "%s: null operand", who);
  scatter_cos_sorted_kernel<<<(unsigned)((n_rows + SBR_SORTED_WAVES - 1) / SBR_SORTED_WAVES), 64 * SBR_SORTED_WAVES, 0, (hipStream_t)stream>>>(
      coef_a, coef_s, src, V, sorted_keys, order, n_slots, slots_per_row, grad, dst, n_rows, D);
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}
