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
// kernel's and is a small fraction of that. D = 256 would need 192 VGPRs for the user planes alone and is not built (the host falls
// back to the fp32 GEMM route).
//
// Everything after the MFMAs is the fp16 kernel's, unchanged: exclusion event stream (s5_build_events, 32-item tiles), unit plan
// with partial waves (s5_plan with F3_MAXW slots), prefix pass and class-maxima thresholds, branch-free appends into the candidate
// buffers, overflow selection, and the final selection kernel (score_topk_cand.h). Validity is gated by index, never by a score
// sentinel: a lane of a user row >= Bu scores a copy of row Bu - 1 (the read is clamped, so no lane reads past the user matrix) into
// buffer rows of its own that the final selection never visits (it runs for rows < Bu only); item columns >= I are set to -inf
// before the threshold compare and the loader clamps their rows to I - 1.
#include "score_topk_cand.h"
#include "gemm_split_common.h"

#define F3_MAXW 7                        // consumer wave slots per workgroup (+ 1 loader wave = 8 waves: two per SIMD)
#define F3_NJ 1                          // 32-item accumulator tiles per LDS tile
#ifndef F3_PRE_TILES
#define F3_PRE_TILES 32                  // prefix-pass tiles (the fp16 kernel's 1,024 items) of catalogues of >= 192 tiles
#endif
#ifndef F3_PF
#define F3_PF 1                          // fragment prefetch distance in K steps (register ring of F3_PF + 1 steps of three fragments)
#endif
#ifndef F3_RF
#define F3_RF 32                         // tiles between two threshold refreshes in the steady state
#endif

template <int KS, int NS, bool PRE>   // KS = D / 16; NS = LDS ring slots (each: three planes of one 32-item tile)
__global__ __launch_bounds__(512) void score_topk_f32s_kernel(
    const float* __restrict__ U, const __bf16* __restrict__ It, long Bu, int I, const unsigned int* __restrict__ events,
    const int* __restrict__ group_base, int item_offset, int k, int n_pre, int W, int n_part, int P,
    int* __restrict__ cnt_out, unsigned long long* __restrict__ gbuf) {
  constexpr int NJ = F3_NJ;
  constexpr int D = KS * 16;
  constexpr int ST_TILE = 32 * NJ;
  constexpr int LIMIT = S5_CAPH - 16 * NJ;                 // a tile adds at most 16 NJ entries to a (user, half) buffer
  constexpr int ROWB = D * 2;
  constexpr int PLANEB = ST_TILE * ROWB;                   // one plane of a tile in LDS
  constexpr int TILEB = 3 * PLANEB;
  constexpr int CPR = D / 8;
  constexpr int SWZ = (CPR >= 16) ? 15 : (CPR - 1);
  constexpr int PER_P = (ST_TILE * CPR) / 64;              // LDS-DMA instructions per plane of a tile
  constexpr int PER_T = 3 * PER_P;
  constexpr int LFL0 = NS - 2 >= 1 ? NS - 2 : 1;           // tiles in flight of the loader wave
  constexpr int LFL = LFL0 * PER_T <= 63 ? LFL0 : 63 / PER_T;
  static_assert(LFL >= 1 && LFL * PER_T <= 63, "vmcnt field");
  static_assert(LIMIT >= 32, "k <= 32 entries must fit below the compaction limit");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  lds_int* full_lds = (lds_int*)(smem + NS * TILEB);
  lds_int* free_lds = full_lds + NS;

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  // work units and partial waves: score_topk_f16_n_kernel
  const int Wb = W + ((int)blockIdx.x < n_part ? 1 : 0);
  const bool partial = wave == W && (int)blockIdx.x < n_part;
  const int part = partial ? (int)blockIdx.x % P : 0, n_parts = partial ? P : 1;
  const long n_full_units = (long)gridDim.x * W;
  const long unit = partial ? n_full_units + (int)blockIdx.x / P : (long)blockIdx.x * W + wave;
  const long n_units = (Bu + 31) >> 5;
  const long brow0 = partial ? n_units * 32 + (long)blockIdx.x * 32 : unit * 32;
  const int n_tiles = (I + ST_TILE - 1) / ST_TILE;
  const int n_virt = n_pre + n_tiles;

  if (t < NS) { full_lds[t] = 0; free_lds[t] = 0; }
  __syncthreads();                                         // the only workgroup barrier of the kernel

  const int cslots = W + (n_part > 0 ? 1 : 0);
  if (wave == W && n_part > 0 && !partial) return;
  if (wave >= cslots) {
    // ---------------------------------------------- loader wave ------------------------------------------------------
    const long plane_stride = (long)I * D;
    int n_mine = 0, v_last = -1;
    for (int v = 0; v < n_virt; ++v) {
      const int slot = v % NS;
      if (v >= NS) {
        const int need = Wb * (v / NS);
        while (st_peek(free_lds + slot) < need) __builtin_amdgcn_s_sleep(1);
      }
      const int j0 = (v < n_pre ? v : v - n_pre) * ST_TILE;
      unsigned char* dst = smem + slot * TILEB;
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int q = 0; q < PER_P; ++q) {
          const int c = q * 64 + lane;
          const int i = c / CPR, cp = c % CPR;
          int gi = j0 + i;
          gi = gi < I ? gi : I - 1;
          const __bf16* src = It + p * plane_stride + (long)gi * D + ((cp ^ (i & SWZ)) << 3);
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                           (__attribute__((address_space(3))) void*)(dst + p * PLANEB + q * 1024), 16, 0, 0);
        }
      }
      v_last = v;
      if (++n_mine > LFL) {
        st_wait_vmcnt<LFL * PER_T>();
        st_wave_fence();
        const int vp = v - LFL;
        *(volatile lds_int*)(full_lds + vp % NS) = vp + 1;
      }
    }
    st_wait_vmcnt<0>();
    st_wave_fence();
    if (v_last >= 0) {
      int vp = v_last - (LFL - 1);
      if (vp < 0) vp = 0;
      for (; vp <= v_last; ++vp) *(volatile lds_int*)(full_lds + vp % NS) = vp + 1;
    }
    return;
  }

  // ------------------------------------------------ consumer waves ------------------------------------------------------
  // B-operand planes of the wave's 32-user tile: user unit * 32 + l31, k = 16 s + 8 half + j, split from fp32 in registers
  sp_u32x4 u0[KS], u1[KS], u2[KS];
  {
    const long r = unit * 32 + l31;
    const long ur = r < Bu ? r : Bu - 1;                   // rows >= Bu: a copy of the last row (never read back)
    const float4* src = reinterpret_cast<const float4*>(U + ur * D);
#pragma unroll
    for (int s = 0; s < KS; ++s) sp_split8(src[4 * s + 2 * half], src[4 * s + 2 * half + 1], u0[s], u1[s], u2[s]);
    // (named before the tile loop: the wait for these loads must not land inside it, behind the candidate stores)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" ::"v"(u0[s]), "v"(u1[s]), "v"(u2[s]));
  }
  unsigned long long* wgb = gbuf + brow0 * (2 * S5_CAPH);
  const i32x4 wrs = s5_block_rsrc(wgb);
  // exclusion event stream: score_topk_f16_n_kernel
  const bool has_excl = events != nullptr && unit < n_units;
  typedef const __attribute__((address_space(4))) unsigned int* ev_ptr;
  typedef unsigned int ev_quad __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(4))) ev_quad* ev_quad_ptr;
  ev_ptr evp = nullptr;
  unsigned int w0 = S5_EV_NONE, w1 = S5_EV_NONE, w2 = S5_EV_NONE, w3 = S5_EV_NONE, n0 = S5_EV_NONE, n1 = S5_EV_NONE, n2 = S5_EV_NONE, n3 = S5_EV_NONE;
  int ev_rem = 4, ev_q = 8;
#define F3_EV_RESTART()                                                                                                  \
  if (has_excl) {                                                                                                        \
    const ev_quad qa = *(ev_quad_ptr)(evp), qb = *(ev_quad_ptr)(evp + 4);                                                \
    w0 = qa.x; w1 = qa.y; w2 = qa.z; w3 = qa.w; n0 = qb.x; n1 = qb.y; n2 = qb.z; n3 = qb.w;                             \
    ev_rem = 4; ev_q = 8;                                                                                                \
  }
  if (has_excl) evp = (ev_ptr)events + ((const __attribute__((address_space(4))) int*)group_base)[unit];
  F3_EV_RESTART()
  int peek = 0;
  int slot_next = 0;
  float thr = -INFINITY;
  const int lane_base = (l31 * 2 + half) * S5_CAPH * 8;
  int pos = lane_base;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

#define F3_EV_NEXT()                                                                                                     \
        w0 = w1; w1 = w2; w2 = w3;                                                                                       \
        if (--ev_rem == 0) {                                                                                             \
          w0 = n0; w1 = n1; w2 = n2; w3 = n3;                                                                            \
          const ev_quad qn = *(ev_quad_ptr)(evp + ev_q);                                                                 \
          n0 = qn.x; n1 = qn.y; n2 = qn.z; n3 = qn.w;                                                                    \
          ev_rem = 4; ev_q += 4;                                                                                         \
        }
#define F3_TILE_SKIP(V, J0)                                                                                              \
  {                                                                                                                      \
    const int slot = slot_next;                                                                                          \
    slot_next = slot + 1 == NS ? 0 : slot + 1;                                                                           \
    while (st_peek(full_lds + slot) != (V) + 1) __builtin_amdgcn_s_sleep(1);                                             \
    st_wave_fence();                                                                                                     \
    s5_lds_add_lane0(free_lds + slot, 1);                                                                                \
    peek = 0;                                                                                                            \
    if (has_excl) {                                                                                                      \
      const unsigned int tkey = (unsigned int)((J0) / ST_TILE);                                                          \
      while ((w0 >> 11) == tkey) { F3_EV_NEXT() }                                                                        \
    }                                                                                                                    \
  }
  // one item tile: wait, six MFMAs per K step (smallest terms first, as gemm_split_f32.hip), slot release, exclusion bits -> ex
#define F3_TILE_BODY(V)                                                                                                  \
    const int slot = slot_next;                                                                                          \
    slot_next = slot + 1 == NS ? 0 : slot + 1;                                                                           \
    if (__builtin_amdgcn_readfirstlane(peek) != (V) + 1) {                                                               \
      while (st_peek(full_lds + slot) != (V) + 1) __builtin_amdgcn_s_sleep(1);                                           \
    }                                                                                                                    \
    st_wave_fence();                                                                                                     \
    f32x16 acc;                                                                                                          \
    sp_u32x4 bf[F3_PF + 1][3];                                                                                           \
    const unsigned char* rowp = smem + slot * TILEB + l31 * ROWB;                                                        \
    unsigned int lxh = (unsigned int)(((l31 & SWZ) << 4) ^ (half << 4));                                                 \
    asm volatile("" : "+v"(lxh));                                                                                        \
    _Pragma("unroll") for (int s = 0; s < F3_PF && s < KS; ++s) {                                                        \
      _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                                      \
        bf[s][p] = *reinterpret_cast<const sp_u32x4*>(rowp + p * PLANEB + (((unsigned int)s << 5) ^ lxh));               \
    }                                                                                                                    \
    if constexpr (S5_PRIO != 0) __builtin_amdgcn_s_setprio(S5_PRIO);                                                     \
    _Pragma("unroll") for (int s = 0; s < KS; ++s) {                                                                     \
      if (s + F3_PF < KS) {                                                                                              \
        _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                                    \
          bf[(s + F3_PF) % (F3_PF + 1)][p] = *reinterpret_cast<const sp_u32x4*>(rowp + p * PLANEB + (((unsigned int)(s + F3_PF) << 5) ^ lxh)); \
      }                                                                                                                  \
      if (s == KS / 2) peek = *(volatile lds_int*)(full_lds + slot_next);                                                \
      __builtin_amdgcn_sched_barrier(0);                                                                                 \
      const sp_u32x4* b = bf[s % (F3_PF + 1)];                                                                           \
      acc = sp_mfma(b[2], u0[s], s == 0 ? zero16 : acc);                                                                 \
      acc = sp_mfma(b[0], u2[s], acc);                                                                                   \
      acc = sp_mfma(b[1], u1[s], acc);                                                                                   \
      acc = sp_mfma(b[1], u0[s], acc);                                                                                   \
      acc = sp_mfma(b[0], u1[s], acc);                                                                                   \
      acc = sp_mfma(b[0], u0[s], acc);                                                                                   \
      __builtin_amdgcn_sched_barrier(0);                                                                                 \
    }                                                                                                                    \
    if constexpr (S5_PRIO != 0) __builtin_amdgcn_s_setprio(0);                                                           \
    s5_lds_done(acc, acc);                                                                                               \
    s5_lds_add_lane0(free_lds + slot, 1);                                                                                \
    unsigned int ex = 0u;                                                                                                \
    bool have_ex = false;                                                                                                \
    if (has_excl) {                                                                                                      \
      const unsigned int tkey = (unsigned int)(j0 / ST_TILE);                                                            \
      while ((w0 >> 11) == tkey) {                                                                                       \
        ex |= lane == (int)((w0 >> 5) & 63u) ? 1u << (w0 & 31u) : 0u;                                                    \
        have_ex = true;                                                                                                  \
        F3_EV_NEXT()                                                                                                     \
      }                                                                                                                  \
    }                                                                                                                    \
    if (j0 + ST_TILE > I) {                                /* catalogue end inside the tile: padded columns never count */ \
      const int lim = I - j0 - 4 * half;                   /* item (r & 3) + 8 (r >> 2) of this lane exists iff < lim */   \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                                   \
        const bool in = (r & 3) + 8 * (r >> 2) < lim;                                                                    \
        acc[r] = in ? acc[r] : -INFINITY;                                                                                \
      }                                                                                                                  \
    }

  // ---- pass 1: prefix tiles, running maximum per accumulator register (item class) -> first threshold ----
  float cm[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) cm[r] = -INFINITY;
  if (partial) {
    for (int v = 0; v < n_pre; ++v) F3_TILE_SKIP(v, v * ST_TILE)
    F3_EV_RESTART()
  } else if (PRE && n_pre > 0) {
    for (int v = 0; v < n_pre; ++v) {
      const int j0 = v * ST_TILE;
      F3_TILE_BODY(v)
      if (have_ex) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = ((ex >> r) & 1u) ? -INFINITY : acc[r];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) cm[r] = fmaxf(cm[r], acc[r]);
    }
    {
      // one step below the k-th largest class maximum (see score_topk_f16_n_kernel: scores equal to the bound must pass, and the
      // step below +0.0 is the negative denormal, not -0.0)
      const float tk = s5_kth_of_32(cm, k);
      const unsigned int key = st_f2key(tk);
      unsigned int below = key - 1u;
      below = below == 0x7FFFFFFFu ? 0x7FFFFFFEu : below;
      thr = key > 0x007FFFFFu ? st_key2f(below) : -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) cm[r] = -INFINITY;
    F3_EV_RESTART()
  }

  // ---- pass 2: all tiles, lane-local threshold filter and appends ----
  const int pos_limit = lane_base + LIMIT * 8;
  int next_rf = (n_pre > 0 && !partial) ? F3_RF - 1 : 0;
  int part_next = part;
  for (int tl = 0; tl < n_tiles; ++tl) {
    if (tl != part_next) {
      F3_TILE_SKIP(n_pre + tl, tl * ST_TILE)
      continue;
    }
    part_next += n_parts;
    if (__ballot(pos > pos_limit)) {
      // overflow (cold): a (user, half) buffer is nearly full — select that user's k best so that this tile's appends fit
      unsigned long long need = __ballot(pos > pos_limit);
      need = (need | (need >> 32)) & 0xFFFFFFFFull;
      const int cnt = (pos - lane_base) >> 3;
      while (need) {
        const int u = __ffsll((long long)need) - 1;
        need &= need - 1ull;
        const int c0 = __builtin_amdgcn_readlane(cnt, u), c1 = __builtin_amdgcn_readlane(cnt, u + 32);
        unsigned long long* b0 = wgb + (long)u * (2 * S5_CAPH);
        const float nt = s5_overflow_select(b0, b0 + S5_CAPH, c0, c1, k, lane);
        if (c0 + c1 >= k && l31 == u) {
          thr = nt > thr ? nt : thr;
          pos = lane_base + (half ? (k >> 1) : k - (k >> 1)) * 8;
        }
      }
    }
    const int j0 = tl * ST_TILE;
    F3_TILE_BODY(n_pre + tl)
    const unsigned int item_lane = 0xFFFFFFFFu - (unsigned int)(item_offset + j0 + 4 * half);
    // threshold ladder: all vector compares first, then scalar dispatch per register pair (score_topk_f16_n_kernel)
    unsigned long long gm[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) gm[g] = __ballot(s5_max2(acc[2 * g], acc[2 * g + 1]) > thr);
    unsigned long long any_g = 0ull;
#pragma unroll
    for (int i = 0; i < 8; ++i) any_g |= gm[i];
    if (any_g) {
#define F3_PAIR(G)                                                                                                       \
      if (__builtin_expect(gm[(G)] != 0ull, 0)) {                                                                        \
        s5_try_append<(1u << (2 * (G))), ((2 * (G)) & 3) + 8 * ((2 * (G)) >> 2), true, false, 2 * (G)>(acc[2 * (G)], thr, ex, pos, item_lane, wrs, cm[2 * (G)], 0u); \
        s5_try_append<(1u << (2 * (G) + 1)), ((2 * (G) + 1) & 3) + 8 * ((2 * (G) + 1) >> 2), true, false, 2 * (G) + 1>(acc[2 * (G) + 1], thr, ex, pos, item_lane, wrs, cm[2 * (G) + 1], 0u); \
      }
      F3_PAIR(0) F3_PAIR(1) F3_PAIR(2) F3_PAIR(3) F3_PAIR(4) F3_PAIR(5) F3_PAIR(6) F3_PAIR(7)
#undef F3_PAIR
    }
    (void)have_ex;
    if (tl >= next_rf) {
      const float tk = s5_kth_of_32(cm, k);
      thr = tk > thr ? tk : thr;
      const int gap = (tl + 2) >> 1;
      next_rf = tl + (gap < F3_RF ? gap : F3_RF);
    }
  }
#undef F3_TILE_BODY
#undef F3_TILE_SKIP
#undef F3_EV_NEXT
#undef F3_EV_RESTART
  {
    int2 o;
    o.x = (pos - lane_base) >> 3;
    o.y = (int)__float_as_uint(thr);
    reinterpret_cast<int2*>(cnt_out)[(brow0 + l31) * 2 + half] = o;
  }
}

__global__ __launch_bounds__(256) void score_topk_f32s_finalize_kernel(long Bu, int k, long n_full_units, int P, const int* __restrict__ cnt,
                                                                       const unsigned long long* __restrict__ gbuf, float* __restrict__ out_val,
                                                                       int* __restrict__ out_idx) {
  s5_finalize(Bu, k, n_full_units, P, cnt, gbuf, out_val, out_idx);
}

static long f3_padded_users(long Bu) { return sbr_cdiv(Bu, 32) * 32 + 32L * F3_MAXW + 32L * s5_n_cu(); }     // as s5_padded_users
static long f3_workspace_bytes(long Bu) {
  const long padded = f3_padded_users(Bu);
  return padded * 2 * S5_CAPH * 8 + s5_al16(padded * 2 * 8);   // candidate buffers + fill counts / final thresholds
}

template <int KS, int NS>
static int f3_launch(const float* U, const void* It, long Bu, int I, const long* u_idx, const long* eptr, const int* eidx, long excl_nnz,
                     int item_offset, int k, float* out_val, int* out_idx, void* workspace, long workspace_bytes, void* ev_buf,
                     long ev_bytes, int build_events, hipStream_t s) {
  const S5Plan plan = s5_plan(Bu, F3_MAXW);
  const int W = plan.W;
  const long n_wg = plan.n_wg;
  const long padded = f3_padded_users(Bu);
  const long buf_bytes = padded * 2 * S5_CAPH * 8;
  SBR_REQUIRE(W + (plan.n_part > 0 ? 1 : 0) <= F3_MAXW, "sbr_score_topk_f32s: internal: wave count");
  SBR_REQUIRE(n_wg * 32L * W + 32L * plan.n_part <= padded && sbr_cdiv(Bu, 32) * 32 + 32L * plan.n_part <= padded, "sbr_score_topk_f32s: internal: padding");
  SBR_REQUIRE(workspace && workspace_bytes >= f3_workspace_bytes(Bu),
              "sbr_score_topk_f32s: workspace of %ld bytes needed (sbr_score_topk_f32s_workspace), %ld given", f3_workspace_bytes(Bu), workspace_bytes);
  int* cnt = (int*)((char*)workspace + buf_bytes);
  const bool with_excl = eptr != nullptr && excl_nnz > 0;
  S5Events evs = {nullptr, nullptr};
  if (with_excl) {
    const int rc = s5_build_events(ev_buf, ev_bytes, Bu, I, u_idx, eptr, eidx, excl_nnz, item_offset, 32 * F3_NJ, build_events != 0, &evs, s);
    if (rc) return rc;
  }
  const size_t lds = (size_t)NS * 3 * (32 * F3_NJ) * KS * 32 + 2 * NS * 4;
  SBR_REQUIRE(lds <= 160 * 1024, "sbr_score_topk_f32s: LDS budget exceeded (%zu bytes)", lds);
  const int n_tiles = sbr_cdiv(I, 32 * F3_NJ);
  const int n_pre = n_tiles >= 6 * F3_PRE_TILES ? F3_PRE_TILES : 0;
  auto kern = score_topk_f32s_kernel<KS, NS, true>;
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    sbr_set_error("sbr_score_topk_f32s: cannot raise the dynamic LDS limit to %zu", lds);
    return SBR_ERR_HIP;
  }
  kern<<<(unsigned int)n_wg, (W + (plan.n_part > 0 ? 1 : 0) + 1) * 64, lds, s>>>(U, (const __bf16*)It, Bu, I, evs.events, evs.group_base, item_offset, k,
                                                                          n_pre, W, plan.n_part, plan.P, cnt, (unsigned long long*)workspace);
  SBR_CHECK_LAUNCH("sbr_score_topk_f32s");
  score_topk_f32s_finalize_kernel<<<(unsigned int)sbr_cdiv(Bu, 4), 256, 0, s>>>(Bu, k, plan.n_part > 0 ? (long)n_wg * W : (1L << 40), plan.P, cnt,
                                                                                (const unsigned long long*)workspace, out_val, out_idx);
  SBR_CHECK_LAUNCH("sbr_score_topk_f32s (final selection)");
  return SBR_OK;
}

extern "C" long sbr_score_topk_f32s_workspace(long Bu, int I, int k) {
  (void)I; (void)k;
  return f3_workspace_bytes(Bu);
}

// U: fp32 [Bu, D] rows; I_bf16x3: the three planes of sbr_split_f32_to_bf16x3 of the fp32 [I, D] item matrix. Events: the protocol
// of sbr_score_topk_f16 and a buffer of sbr_score_topk_f16_events_bytes(Bu, excl_nnz) bytes, but a stream built by THIS entry
// (32-item tiles): the fp16 route's stream of the same users is laid out for its own tile width and must not be handed over.
extern "C" int sbr_score_topk_f32s(const float* U, const void* I_bf16x3, int D, long Bu, int I, const long* u_idx,
                                   const long* excl_indptr, const int* excl_indices, long excl_nnz, int item_offset, int k, float* out_val,
                                   int* out_idx, void* workspace, long workspace_bytes, void* events, long events_bytes, int build_events,
                                   void* stream) {
  SBR_REQUIRE(k >= 1 && k <= 32, "sbr_score_topk_f32s: k=%d outside [1, 32] (use sbr_gemm_f32 + sbr_topk_rows)", k);
  SBR_REQUIRE(I >= 1, "sbr_score_topk_f32s: empty catalogue");
  SBR_REQUIRE(D == 64 || D == 128, "sbr_score_topk_f32s: D=%d not supported (64, 128)", D);
  if (Bu == 0) return SBR_OK;
  SBR_REQUIRE(U && I_bf16x3 && out_val && out_idx, "sbr_score_topk_f32s: null operand");
  SBR_REQUIRE(((size_t)U & 15) == 0 && ((size_t)I_bf16x3 & 15) == 0, "sbr_score_topk_f32s: operands must be 16-byte aligned");
  SBR_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), "sbr_score_topk_f32s: exclusion CSR must be given whole or not at all");
  const hipStream_t s = (hipStream_t)stream;
  if (D == 64)
    return f3_launch<4, 12>(U, I_bf16x3, Bu, I, u_idx, excl_indptr, excl_indices, excl_nnz, item_offset, k, out_val, out_idx, workspace,
                            workspace_bytes, events, events_bytes, build_events, s);
  return f3_launch<8, 6>(U, I_bf16x3, Bu, I, u_idx, excl_indptr, excl_indices, excl_nnz, item_offset, k, out_val, out_idx, workspace,
                         workspace_bytes, events, events_bytes, build_events, s);
}

// X (fp32, n elements) -> Y = three bf16 planes of n elements each, X = Y[0] + Y[1] + Y[2] exactly (round to nearest even per plane)
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
