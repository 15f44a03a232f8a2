// Fused full-catalogue scorer with fp32-class products (eval/eval.py:216-222: scores = U x I^T in fp32, out[excluded] = -inf,
// top-k; the score matrix is never written). The one-pass kernel of score_topk_f16_n.hip with its operands on the bf16 matrix pipe
// over exact three-way splits instead of rounded to fp16.
//
// Arithmetic (gemm_split_f32.hip, header): an fp32 number is the exact sum of three bf16 numbers, x = x0 + x1 + x2, and the six
// leading partial products sum_{i + j <= 2} i_i u_j (products exact, fp32 accumulation) give u . i to within the fp32 pipe's own
// rounding class (|dropped| <= 2^-23 |u_d i_d| per term). Six v_mfma_f32_32x32x16_bf16 per 16-deep K step replace the fp16 kernel's one.
//
// Operands. The ITEM side is split once per evaluation (sbr_split_f32_to_bf16x3: three planes [3][I][D] of bf16, each laid out like
// the fp16 kernel's item matrix) and streamed by the loader wave into the LDS ring: a slot holds the three planes of one 32-item tile
// (24 KB at D = 128), each with the fp16 kernel's XOR swizzle. Every workgroup streams the whole catalogue, 3x the fp16 route's bytes
// (38 MB per workgroup pass at 50k x 128), about 12 GB/s per CU at the measured pass time: inside one loader wave's rate.
// The USER side is read once per wave in fp32 and split in registers (sp_split8), as the split GEMM splits its A rows: 3 x D / 16 x 4
// VGPRs (96 at D = 128) for the wave's 32 users.
//
// Geometry. The user planes do not fit the fp16 kernel's 128-register budget (four waves per SIMD), so a workgroup is 8 waves (two per
// SIMD, up to 256 registers each): up to 7 consumer waves + 1 loader wave. Per 32-item tile a consumer wave at D = 128 issues
// 6 x 8 = 48 MFMAs (~1,540 cycles) against three ds_read_b128 per K step; the compare / append / threshold work per tile is the fp16
// kernel's and is a small fraction of that. D = 256 needs 192 VGPRs for the user planes alone: it does not fit this geometry and has
// kernels of its own below (one wave per SIMD; sbr_score_topk_f32s_d256), sbr_score_topk_f32s keeps refusing it.
//
// Everything but the operands is the fp16 kernel's: the kernel is st_one_pass (score_topk_stream.h) with the StF32s operand policy —
// exclusion event stream (s5_build_events, 32-item tiles), unit plan with partial waves (s5_plan with F3_MAXW slots), prefix pass and
// class-maxima thresholds, branch-free appends into the candidate buffers, overflow selection, and the final selection kernel
// (score_topk_finalize_kernel). Validity is gated by index, never by a score
// sentinel: a lane of a user row >= Bu scores a copy of row Bu - 1 (the read is clamped, so no lane reads past the user matrix) into
// buffer rows of its own that the final selection never visits (it runs for rows < Bu only); item columns >= I are set to -inf
// before the threshold compare and the loader clamps their rows to I - 1.
#include "score_topk_stream.h"
#include "gemm_split_common.h"

#define F3_MAXW 7                        // consumer wave slots per workgroup (+ 1 loader wave = 8 waves: two per SIMD)
#ifndef F3_PRE_TILES
#define F3_PRE_TILES 32                  // prefix-pass tiles (the fp16 kernel's 1,024 items) of catalogues of >= 192 tiles
#endif
#ifndef F3_PF
#define F3_PF 1                          // fragment prefetch distance in K steps (register ring of F3_PF + 1 steps of three fragments)
#endif

// operand policy of st_one_pass (score_topk_stream.h): fp32 user rows split in registers, three bf16 item planes per ring tile, six
// MFMAs per K step (smallest terms first, as gemm_split_f32.hip)
template <int KS_, int MAXW_ = F3_MAXW>
struct StF32s {
  static constexpr int KS = KS_, NJ = 1, PLANES = 3, NF = 3;
  static constexpr int MAXW = MAXW_, NL = 1, PRE_TILES = F3_PRE_TILES;
  static constexpr int PF = F3_PF, PF_PRE = F3_PF;
  typedef float UT;
  typedef __bf16 IT;
  typedef sp_u32x4 Frag;
  sp_u32x4 u0[KS], u1[KS], u2[KS];                         // B operand planes: user row, k = 16 s + 8 half + j
  __device__ __forceinline__ void load_users(const float* U, long ur, int half) {
    const float4* src = reinterpret_cast<const float4*>(U + ur * (KS * 16));
#pragma unroll
    for (int s = 0; s < KS; ++s) sp_split8(src[4 * s + 2 * half], src[4 * s + 2 * half + 1], u0[s], u1[s], u2[s]);
    // (named before the tile loop: the wait for these loads must not land inside it, behind the candidate stores)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" ::"v"(u0[s]), "v"(u1[s]), "v"(u2[s]));
  }
  // b[p]: plane p of the item fragment
  __device__ __forceinline__ void mma(f32x16 (&acc)[1], const sp_u32x4 (&b)[3], int s) const {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    acc[0] = sp_mfma(b[2], u0[s], s == 0 ? zero16 : acc[0]);
    acc[0] = sp_mfma(b[0], u2[s], acc[0]);
    acc[0] = sp_mfma(b[1], u1[s], acc[0]);
    acc[0] = sp_mfma(b[1], u0[s], acc[0]);
    acc[0] = sp_mfma(b[0], u1[s], acc[0]);
    acc[0] = sp_mfma(b[0], u0[s], acc[0]);
  }
};

template <int KS, int NS>   // KS = D / 16; NS = LDS ring slots (each: three planes of one 32-item tile)
__global__ __launch_bounds__(512) void score_topk_f32s_kernel(
    const float* __restrict__ U, const __bf16* __restrict__ It, long Bu, int I, const unsigned int* __restrict__ events,
    const int* __restrict__ group_base, int item_offset, int k, int n_pre, int W, int n_part, int P,
    int* __restrict__ cnt_out, unsigned long long* __restrict__ gbuf) {
  st_one_pass<StF32s<KS>, NS>(U, It, Bu, I, events, group_base, item_offset, k, n_pre, W, n_part, P, cnt_out, gbuf);
}

// the wide instantiation (33 <= k <= 128, st_one_pass<..., WIDE>): a kernel of its own, chosen on the host by k > 32
template <int KS, int NS>
__global__ __launch_bounds__(512) void score_topk_wide_f32s_kernel(
    const float* __restrict__ U, const __bf16* __restrict__ It, long Bu, int I, const unsigned int* __restrict__ events,
    const int* __restrict__ group_base, int item_offset, int k, int n_pre, int W, int n_part, int P,
    int* __restrict__ cnt_out, unsigned long long* __restrict__ gbuf) {
  st_one_pass<StF32s<KS>, NS, true>(U, It, Bu, I, events, group_base, item_offset, k, n_pre, W, n_part, P, cnt_out, gbuf);
}

// D = 256: the user planes take 192 registers, so a workgroup is 4 waves, one per SIMD with the whole 512-entry register file each:
// F3W_MAXW consumer waves + 1 loader wave over a ring of 3 slots of 48 KB. Kernels of their own names: the set of
// instantiations of the two kernels above stays what it is.
#define F3W_MAXW 3
#define F3W_NS 3
typedef StF32s<16, F3W_MAXW> StF32sD256;

__global__ __launch_bounds__(256) void score_topk_f32s_d256_kernel(
    const float* __restrict__ U, const __bf16* __restrict__ It, long Bu, int I, const unsigned int* __restrict__ events,
    const int* __restrict__ group_base, int item_offset, int k, int n_pre, int W, int n_part, int P,
    int* __restrict__ cnt_out, unsigned long long* __restrict__ gbuf) {
  st_one_pass<StF32sD256, F3W_NS>(U, It, Bu, I, events, group_base, item_offset, k, n_pre, W, n_part, P, cnt_out, gbuf);
}

__global__ __launch_bounds__(256) void score_topk_wide_f32s_d256_kernel(
    const float* __restrict__ U, const __bf16* __restrict__ It, long Bu, int I, const unsigned int* __restrict__ events,
    const int* __restrict__ group_base, int item_offset, int k, int n_pre, int W, int n_part, int P,
    int* __restrict__ cnt_out, unsigned long long* __restrict__ gbuf) {
  st_one_pass<StF32sD256, F3W_NS, true>(U, It, Bu, I, events, group_base, item_offset, k, n_pre, W, n_part, P, cnt_out, gbuf);
}

extern "C" long sbr_score_topk_f32s_workspace(long Bu, int I, int k) {
  (void)I; (void)k;
  return st_workspace_bytes(Bu, F3_MAXW);
}

// U: fp32 [Bu, D] rows; I_bf16x3: the three planes of sbr_split_f32_to_bf16x3 of the fp32 [I, D] item matrix. Events: the protocol
// of sbr_score_topk_f16 and a buffer of sbr_score_topk_f16_events_bytes(Bu, excl_nnz) bytes, but a stream built by THIS entry
// (32-item tiles): the fp16 route's stream of the same users is laid out for its own tile width and must not be handed over.
extern "C" int sbr_score_topk_f32s(const float* U, const void* I_bf16x3, int D, long Bu, int I, const long* u_idx,
                                   const long* excl_indptr, const int* excl_indices, long excl_nnz, int item_offset, int k, float* out_val,
                                   int* out_idx, void* workspace, long workspace_bytes, void* events, long events_bytes, int build_events,
                                   void* stream) {
  SBR_REQUIRE(k >= 1 && k <= 128, "sbr_score_topk_f32s: k=%d outside [1, 128] (use sbr_gemm_f32 + sbr_topk_rows)", k);
  SBR_REQUIRE(I >= 1, "sbr_score_topk_f32s: empty catalogue");
  SBR_REQUIRE(D == 64 || D == 128, "sbr_score_topk_f32s: D=%d not supported (64, 128)", D);
  if (Bu == 0) return SBR_OK;
  SBR_REQUIRE(U && I_bf16x3 && out_val && out_idx, "sbr_score_topk_f32s: null operand");
  SBR_REQUIRE(((size_t)U & 15) == 0 && ((size_t)I_bf16x3 & 15) == 0, "sbr_score_topk_f32s: operands must be 16-byte aligned");
  SBR_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), "sbr_score_topk_f32s: exclusion CSR must be given whole or not at all");
  const hipStream_t s = (hipStream_t)stream;
  const __bf16* It = (const __bf16*)I_bf16x3;
  if (k > 32) {                                              // the wide instantiations: lists of 33 .. 128
    if (D == 64)
      return st_launch<StF32s<4>, 12, true>(score_topk_wide_f32s_kernel<4, 12>, "sbr_score_topk_f32s", U, It, Bu, I, u_idx, excl_indptr, excl_indices,
                                            excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, events, events_bytes, build_events, s);
    return st_launch<StF32s<8>, 6, true>(score_topk_wide_f32s_kernel<8, 6>, "sbr_score_topk_f32s", U, It, Bu, I, u_idx, excl_indptr, excl_indices,
                                         excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, events, events_bytes, build_events, s);
  }
  if (D == 64)
    return st_launch<StF32s<4>, 12>(score_topk_f32s_kernel<4, 12>, "sbr_score_topk_f32s", U, It, Bu, I, u_idx, excl_indptr, excl_indices,
                                    excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, events, events_bytes, build_events, s);
  return st_launch<StF32s<8>, 6>(score_topk_f32s_kernel<8, 6>, "sbr_score_topk_f32s", U, It, Bu, I, u_idx, excl_indptr, excl_indices,
                                 excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, events, events_bytes, build_events, s);
}

extern "C" long sbr_score_topk_f32s_d256_workspace(long Bu, int I, int k) {
  (void)I; (void)k;
  return st_workspace_bytes(Bu, F3W_MAXW);
}

// sbr_score_topk_f32s for D = 256 (same operands, same event protocol and stream layout: 32-item tiles)
extern "C" int sbr_score_topk_f32s_d256(const float* U, const void* I_bf16x3, int D, long Bu, int I, const long* u_idx,
                                        const long* excl_indptr, const int* excl_indices, long excl_nnz, int item_offset, int k, float* out_val,
                                        int* out_idx, void* workspace, long workspace_bytes, void* events, long events_bytes, int build_events,
                                        void* stream) {
  SBR_REQUIRE(k >= 1 && k <= 128, "sbr_score_topk_f32s_d256: k=%d outside [1, 128] (use sbr_gemm_f32 + sbr_topk_rows)", k);
  SBR_REQUIRE(I >= 1, "sbr_score_topk_f32s_d256: empty catalogue");
  SBR_REQUIRE(D == 256, "sbr_score_topk_f32s_d256: D=%d not supported (256; sbr_score_topk_f32s has 64 and 128)", D);
  if (Bu == 0) return SBR_OK;
  SBR_REQUIRE(U && I_bf16x3 && out_val && out_idx, "sbr_score_topk_f32s_d256: null operand");
  SBR_REQUIRE(((size_t)U & 15) == 0 && ((size_t)I_bf16x3 & 15) == 0, "sbr_score_topk_f32s_d256: operands must be 16-byte aligned");
  SBR_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), "sbr_score_topk_f32s_d256: exclusion CSR must be given whole or not at all");
  const hipStream_t s = (hipStream_t)stream;
  const __bf16* It = (const __bf16*)I_bf16x3;
  if (k > 32)
    return st_launch<StF32sD256, F3W_NS, true>(score_topk_wide_f32s_d256_kernel, "sbr_score_topk_f32s_d256", U, It, Bu, I, u_idx, excl_indptr,
                                               excl_indices, excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, events,
                                               events_bytes, build_events, s);
  return st_launch<StF32sD256, F3W_NS>(score_topk_f32s_d256_kernel, "sbr_score_topk_f32s_d256", U, It, Bu, I, u_idx, excl_indptr, excl_indices,
                                       excl_nnz, item_offset, k, out_val, out_idx, workspace, workspace_bytes, events, events_bytes,
                                       build_events, s);
}

// X (fp32, n elements) -> Y = three bf16 planes of n elements each (round to nearest even per plane), X = Y[0] + Y[1] + Y[2] exactly for
// x = 0 and 2^-100 <= |x| <= 3.38e38: below, the third plane (up to 2^-16 |x|) underflows bf16; above ~3.3961e38 the first plane rounds
// to inf and the residual is NaN, as for inf / NaN inputs — the fused fp32-class scorer does not take such item values (ops.py)
__global__ void split_bf16x3_kernel(const float* __restrict__ X, unsigned short* __restrict__ Y, long n) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    unsigned int p0, p1, p2;
    sp_split2(X[e], 0.f, p0, p1, p2);
    Y[e] = (unsigned short)p0;
    Y[n + e] = (unsigned short)p1;
    Y[2 * n + e] = (unsigned short)p2;
  }
}

extern "C" int sbr_split_f32_to_bf16x3(const float* X, void* Y_bf16x3, long n, void* stream) {
  if (n == 0) return SBR_OK;
  SBR_REQUIRE(X && Y_bf16x3, "sbr_split_f32_to_bf16x3: null operand");
  int blocks = sbr_cdiv(n, 256);
  if (blocks > 8192) blocks = 8192;
  split_bf16x3_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(X, (unsigned short*)Y_bf16x3, n);
  SBR_CHECK_LAUNCH("sbr_split_f32_to_bf16x3");
  return SBR_OK;
}
