// Fused full-catalogue scorer, narrow-wave kernel (round 2, second half): 32 users per wave, up to 15 consumer waves + 1 loader
// wave per workgroup = four waves per SIMD. Replaces the transposed 64-users-per-wave kernel of score_topk_f16.hip
// (eval/eval.py:205-222: scores = U x I^T, out[excluded] = -inf, top-k; the score matrix is never written).
//
// Why. The transposed kernel ran two waves per SIMD (240 VGPRs each). A wave is in-order: while it walks its threshold ladder and
// its candidate blocks the matrix pipe only has the SIMD's other wave to draw on, and when both are in their ladders it idles —
// cycle stamps put 55 % of a wave's life in the ladder and the PMC matrix-pipe utilisation at 19 %. Here a wave keeps ONE
// 32-user B fragment set (D / 16 x 4 VGPRs) and 16 NJ accumulators, fits in 128 VGPRs, and four of them share a SIMD: the
// ladder, the candidate blocks and the compactions of three waves hide under the MFMAs of the fourth. The LDS bytes read per
// flop double (a fragment read feeds one MFMA instead of two): 15 x 16 KB per 64-item tile = 940 LDS cycles against 1,920 cycles
// of MFMA per SIMD, still under half the array's rate. The number of consumer waves is a launch parameter: users are dealt in
// 32-user units, so 100k users become 241 workgroups of 13 waves (94 % of the CUs busy for the whole kernel) instead of 224 of
// 7 x 64 (87.5 %).
//
// Kept from the transposed kernel: A = item fragment (LDS ring filled by LDS-DMA, XOR swizzle on the source address, FULL / FREE
// counters per slot, no workgroup barrier in the loop), B = user fragment, so lane (u, h) holds for ONE user the scores of 16
// items of every 32-item tile; lane-local threshold and fill, fire-and-forget appends, cooperative compaction by selection, the
// prefix pass with class maxima, exclusions delivered as bits to the owning lane. New besides the geometry:
//   * the first MFMA of a chain takes the inline constant 0 as C (no accumulator clears: 32 v_mov per tile saved);
//   * a candidate is stored RAW (score bits, ~item) through a buffer descriptor of the wave's 32 KB buffer block at a per-lane
//     byte cursor: the append is one buffer_store_dwordx2 + one v_add, no 64-bit address arithmetic and no key conversion
//     (keys are built at compaction);
//   * thresholds are compared as floats on raw accumulators, ordering / tie rules unchanged (score desc, item index asc).
//
// Round 3: thresholds without compactions. A user's candidate buffers are large (S5_CAPH entries per lane half, in the workspace) and
// are not compacted during the stream; instead every lane keeps the running MAXIMUM of what it appended per accumulator register
// ("class": 16 per lane, 32 per user, updated by one v_max inside the branch-free append, under its EXEC mask — so excluded scores
// and scores below the threshold never enter). The k-th largest of a user's 32 class maxima is the score of a real, already
// buffered item with k - 1 buffered items of other classes at or above it: every later item (larger index) needs a strictly larger
// score to reach the top k. All 32 users of a wave refresh their threshold from it at once, lane-parallel (sort 16 registers by a
// Batcher network, exchange with the partner lane, bitonic half-merge: ~270 vector instructions, no ballots, no memory), every few
// tiles at first and every 32 tiles later. The cooperative per-user selection (s5_select: 32 ballot rounds for ONE user) remains
// only as the overflow path of a (user, half) buffer, and the final selection + ranking runs in a kernel of its own
// (score_topk_finalize_kernel: one wave per user, all CUs busy) instead of serially per user at the tail of the scorer's waves.
#include "score_topk_stream.h"

template <int KS, int NS, int NJ>   // KS = D / 16; NS = LDS ring slots; NJ = 32-item accumulator tiles per LDS tile
__global__ __launch_bounds__(1024) void score_topk_f16_n_kernel(
    const _Float16* __restrict__ U, const _Float16* __restrict__ It, long Bu, int I, const unsigned int* __restrict__ events,
    const int* __restrict__ group_base, int item_offset, int k, int n_pre, int W, int n_part, int P,
    int* __restrict__ cnt_out, unsigned long long* __restrict__ gbuf) {
  st_one_pass<StF16<KS, NJ>, NS>(U, It, Bu, I, events, group_base, item_offset, k, n_pre, W, n_part, P, cnt_out, gbuf);
}

// the wide instantiation (33 <= k <= 128, st_one_pass<..., WIDE>): a kernel of its own, chosen on the host by k > 32 — the kernel above is
// what it was before wide lists existed
template <int KS, int NS, int NJ>
__global__ __launch_bounds__(1024) void score_topk_wide_f16_kernel(
    const _Float16* __restrict__ U, const _Float16* __restrict__ It, long Bu, int I, const unsigned int* __restrict__ events,
    const int* __restrict__ group_base, int item_offset, int k, int n_pre, int W, int n_part, int P,
    int* __restrict__ cnt_out, unsigned long long* __restrict__ gbuf) {
  st_one_pass<StF16<KS, NJ>, NS, true>(U, It, Bu, I, events, group_base, item_offset, k, n_pre, W, n_part, P, cnt_out, gbuf);
}

// final selection of the one-pass kernels' candidate buffers (s5_finalize, score_topk_cand.h), for both routes
__global__ __launch_bounds__(256) void score_topk_finalize_kernel(long Bu, int k, long n_full_units, int P, const int* __restrict__ cnt,
                                                                  const unsigned long long* __restrict__ gbuf, float* __restrict__ out_val,
                                                                  int* __restrict__ out_idx) {
  s5_finalize<false>(Bu, k, n_full_units, P, cnt, gbuf, out_val, out_idx);
}
__global__ __launch_bounds__(256) void score_topk_rank_wide_kernel(long Bu, int k, long n_full_units, int P, const int* __restrict__ cnt,
                                                                       const unsigned long long* __restrict__ gbuf, float* __restrict__ out_val,
                                                                       int* __restrict__ out_idx) {
  s5_finalize<true>(Bu, k, n_full_units, P, cnt, gbuf, out_val, out_idx);
}

extern "C" long sbr_score_topk_f16_events_bytes(long Bu, long excl_nnz) { return s5_event_bytes(Bu, excl_nnz); }

template <int KS, int NS, int NJ>
static int s5_launch(const void* U, const void* It, long Bu, int I, const long* u_idx, const long* eptr, const int* eidx, long excl_nnz,
                     int item_offset, int k, float* out_val, int* out_idx, void* workspace, long workspace_bytes, void* ev_buf,
                     long ev_bytes, int build_events, hipStream_t s) {
  if (k > 32)                                                // the wide instantiation: lists of 33 .. 128
    return st_launch<StF16<KS, NJ>, NS, true>(score_topk_wide_f16_kernel<KS, NS, NJ>, "sbr_score_topk_f16", (const _Float16*)U,
                                              (const _Float16*)It, Bu, I, u_idx, eptr, eidx, excl_nnz, item_offset, k, out_val, out_idx, workspace,
                                              workspace_bytes, ev_buf, ev_bytes, build_events, s);
  return st_launch<StF16<KS, NJ>, NS>(score_topk_f16_n_kernel<KS, NS, NJ>, "sbr_score_topk_f16", (const _Float16*)U, (const _Float16*)It, Bu, I,
                                      u_idx, eptr, eidx, excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, ev_buf,
                                      ev_bytes, build_events, s);
}

// D in {64, 128, 256}
static int s5_dispatch(const void* U, const void* It, int D, long Bu, int I, const long* u_idx, const long* eptr, const int* eidx, long excl_nnz,
                       int item_offset, int k, float* out_val, int* out_idx, void* workspace, long workspace_bytes, void* ev_buf, long ev_bytes,
                       int build_events, hipStream_t s) {
  switch (D) {
    case 64: return s5_launch<4, 8, 2>(U, It, Bu, I, u_idx, eptr, eidx, excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, ev_buf, ev_bytes, build_events, s);
    case 128: return s5_launch<8, S5_NS, 2>(U, It, Bu, I, u_idx, eptr, eidx, excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, ev_buf, ev_bytes, build_events, s);
    case 256: return s5_launch<16, S5_NS, 1>(U, It, Bu, I, u_idx, eptr, eidx, excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, ev_buf, ev_bytes, build_events, s);
    default:
      sbr_set_error("sbr_score_topk_f16: D=%d not supported by the narrow-wave kernel", D);
      return SBR_ERR_ARG;
  }
}

// the two-pass scorer (score_topk_f16_2p.hip)
bool s2_supported(int D, long Bu, int I, int k);
long s2_workspace_bytes(long Bu, int I);
int s2_dispatch(const void* U, const void* It, int D, long Bu, int I, const long* u_idx, const long* eptr, const int* eidx, long excl_nnz,
                int item_offset, int k, float* out_val, int* out_idx, void* workspace, long workspace_bytes, void* ev_buf, long ev_bytes,
                int build_events, hipStream_t s);

// 0: automatic (the one-pass kernel for every shape until the two-pass scorer is the faster one), 1: always the one-pass kernel,
// 2: two-pass (catalogues of >= 8,192 items, k <= 32) or an error.
// Both routes return the same lists bit for bit; the switch exists for tests and A/B timing.
static int g_route = 0;
extern "C" int sbr_score_topk_f16_route(int route) {
  const int prev = g_route;
  if (route >= 0 && route <= 2) g_route = route;
  return prev;
}

// bytes of the workspace of a call on the route selected now: the one-pass kernel's (candidate buffers, fill counts), or under route 2
// the larger of that and the two-pass scorer's (group maxima, pair lists, candidate regions). A call made after the route was switched
// to 2 checks its workspace and fails with an error if it is too small.
extern "C" long sbr_score_topk_f16_workspace(long Bu, int I, int k) {
  const long one = st_workspace_bytes(Bu, S5_MAXW);
  if (g_route != 2) return one;
  const long two = s2_supported(128, Bu, I, k < 1 ? 1 : (k > 32 ? 32 : k)) ? s2_workspace_bytes(Bu, I) : 0;
  return one > two ? one : two;
}

// events / events_bytes: caller-owned buffer of sbr_score_topk_f16_events_bytes(Bu, excl_nnz) bytes (NULL without exclusions);
// build_events != 0: the event stream of (u_idx, exclusion CSR, item range, D) is built into it first (three small launches),
// 0: it holds the stream a previous call with the same (u_idx, CSR, item_offset, I, D) built.
extern "C" int sbr_score_topk_f16(const void* U_f16, const void* I_f16, int D, long Bu, int I, const long* u_idx,
                                  const long* excl_indptr, const int* excl_indices, long excl_nnz, int item_offset, int k, float* out_val,
                                  int* out_idx, void* workspace, long workspace_bytes, void* events, long events_bytes, int build_events,
                                  void* stream) {
  SBR_REQUIRE(k >= 1 && k <= 128, "sbr_score_topk_f16: k=%d outside [1, 128] (use sbr_gemm_f32 + sbr_topk_rows)", k);
  SBR_REQUIRE(I >= 1, "sbr_score_topk_f16: empty catalogue");
  if (Bu == 0) return SBR_OK;
  SBR_REQUIRE(U_f16 && I_f16 && out_val && out_idx, "sbr_score_topk_f16: null operand");
  SBR_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), "sbr_score_topk_f16: exclusion CSR must be given whole or not at all");
  SBR_REQUIRE(D == 64 || D == 128 || D == 256, "sbr_score_topk_f16: D=%d not supported (64, 128, 256)", D);
  SBR_REQUIRE(g_route != 2 || k <= 32, "sbr_score_topk_f16: the two-pass route takes k <= 32 (k=%d); select route 0 or 1 for longer lists", k);
  const bool two = s2_supported(D, Bu, I, k);
  SBR_REQUIRE(g_route != 2 || two, "sbr_score_topk_f16: the two-pass route was requested for a shape it does not take (I=%d)", I);
  if (two && g_route == 2)      // (checkpoint: the automatic route stays on the one-pass kernel until the two-pass scorer is the faster one)
    return s2_dispatch(U_f16, I_f16, D, Bu, I, u_idx, excl_indptr, excl_indices, excl_nnz, item_offset, k, out_val, out_idx, workspace,
                       workspace_bytes, events, events_bytes, build_events, (hipStream_t)stream);
  return s5_dispatch(U_f16, I_f16, D, Bu, I, u_idx, excl_indptr, excl_indices, excl_nnz, item_offset, k, out_val, out_idx, workspace,
                     workspace_bytes, events, events_bytes, build_events, (hipStream_t)stream);
}

__global__ void cast_f16_kernel(const float* __restrict__ X, _Float16* __restrict__ Y, long n) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) Y[e] = (_Float16)X[e];
}

extern "C" int sbr_cast_f32_to_f16(const float* X, void* Y_f16, long n, void* stream) {
  if (n == 0) return SBR_OK;
  SBR_REQUIRE(X && Y_f16, "sbr_cast_f32_to_f16: null operand");
  int blocks = sbr_cdiv(n, 256);
  if (blocks > 8192) blocks = 8192;
  cast_f16_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(X, (_Float16*)Y_f16, n);
  SBR_CHECK_LAUNCH("sbr_cast_f32_to_f16");
  return SBR_OK;
}
