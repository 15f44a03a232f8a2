// The streaming skeleton of the fused scorers: work-unit geometry, the loader wave that fills the LDS tile ring, the exclusion-event
// cursor, the MFMA pass over one ring tile, the one-pass consumer loop (prefix pass, threshold ladder, appends, refreshes) and its host
// launch. score_topk_f16_n.hip (fp16 operands) and score_topk_f32s.hip (fp32 operands split into three bf16 planes) are thin wrappers
// over st_one_pass with an operand policy each; pass 1 of the two-pass scorer (score_topk_f16_2p.hip) reuses the geometry, the loader,
// the cursor and the tile pass. Everything here has internal linkage except score_topk_finalize_kernel (defined in score_topk_f16_n.hip).
//
// An operand policy supplies:
//   KS (= D / 16), NJ (32-item accumulator tiles per ring tile), PLANES (item planes per ring tile), NF (A fragments per K step:
//   fragment f of step s is the 16-byte chunk at rowp + f * 32 rows + (s << 5) ^ lxh), MAXW (consumer wave slots per workgroup),
//   NL (loader waves), PRE_TILES (prefix-pass tiles; the pass runs on catalogues of >= 6 PRE_TILES tiles), PF / PF_PRE (fragment
//   prefetch distance in K steps in the main / prefix pass), the element types UT / IT of the user and item matrices and Frag of a
//   fragment; load_users(U, row, half) and mma(acc, frags of one K step, s).
#pragma once
#include "score_topk_cand.h"
#include <type_traits>

#ifndef S5_PRE_TILES
#define S5_PRE_TILES 16                  // fp16 route: tiles of the prefix pass (class maxima only, no appends) of catalogues of >= 96 tiles
#endif
#ifndef S5_CML_KS
#define S5_CML_KS 16                     // class maxima of the main pass in LDS for D >= 16 * S5_CML_KS (else in registers)
#endif
#ifndef S5_RF
#define S5_RF 32                         // tiles between two threshold refreshes in the steady state
#endif

// ---- work units. A unit = 32 users x the whole catalogue. A workgroup has W FULL consumer waves (unit blockIdx.x * W + wave); when the
// units do not divide evenly over the CUs, the remainder units are each cut into P PARTS by item tile (the one-pass kernels: tile t
// belongs to part t % P; pass 1 of the two-pass scorer: supertile pairs) and workgroup b < n_part gets one more consumer wave for part
// b % P of remainder unit b / P — with its own candidate buffers, merged by the final selection. (One unit more per workgroup instead
// would put a fourth consumer wave on ONE SIMD of every CU: that SIMD's instruction stream sets the pace of the whole workgroup through
// the tile ring — cycle stamps: the other waves waited a quarter of their time.)
struct StUnit {
  int Wb;                                // consumer waves of THIS workgroup
  bool partial;                          // this wave scores a part of a remainder unit (wave-uniform)
  int part, n_parts;
  long n_full_units, unit, n_units;      // unit: 32-user group of this wave
  long brow0;                            // first row of the wave's candidate buffers / fill counts (partial waves: rows behind all units)
  __device__ __forceinline__ StUnit(long Bu, int W, int n_part, int P, int wave)
      : Wb(W + ((int)blockIdx.x < n_part ? 1 : 0)), partial(wave == W && (int)blockIdx.x < n_part), part(partial ? (int)blockIdx.x % P : 0),
        n_parts(partial ? P : 1), n_full_units((long)gridDim.x * W),
        unit(partial ? n_full_units + (int)blockIdx.x / P : (long)blockIdx.x * W + wave), n_units((Bu + 31) >> 5),
        brow0(partial ? n_units * 32 + (long)blockIdx.x * 32 : unit * 32) {}
};

// ---- loader waves. NL waves take the ring tiles in turn (tile v belongs to loader v % NL) and fill a slot of PLANES planes of ST_TILE
// item rows by LDS-DMA (the 16-byte chunk cp of row i lands at chunk cp ^ (i & SWZ): conflict-free fragment reads), after the slot's
// previous tile has been released by all Wb consumer waves (FREE counter); a tile is published through its FULL word once its loads
// have landed. The tile sequence is n_pre prefix tiles (tiles 0 .. n_pre - 1) and then all tiles. One wave's LDS-DMA stream tops out
// near one 16 KB tile per 0.65 us, which is what fourteen fp16 consumer waves eat.
template <int PLANES, int ST_TILE, int D, int NS, int NL, typename T>
__device__ __forceinline__ void st_loader(unsigned char* smem, lds_int* full_lds, lds_int* free_lds, const T* It, int I, int n_pre, int n_virt,
                                          int Wb, int lw, int lane) {
  constexpr int ROWB = D * 2;
  constexpr int PLANEB = ST_TILE * ROWB;
  constexpr int TILEB = PLANES * PLANEB;
  constexpr int CPR = D / 8;
  constexpr int SWZ = (CPR >= 16) ? 15 : (CPR - 1);
  constexpr int PER_P = (ST_TILE * CPR) / 64;              // LDS-DMA instructions per plane of a tile
  constexpr int PER_T = PLANES * PER_P;
  constexpr int LFL0 = (NS - 2) / NL >= 1 ? (NS - 2) / NL : 1;     // tiles in flight per loader wave
  constexpr int LFL = LFL0 * PER_T <= 63 ? LFL0 : 63 / PER_T;
  static_assert(LFL >= 1 && LFL * PER_T <= 63, "vmcnt field");
  const long plane_stride = (long)I * D;
  int n_mine = 0, v_last = -1;
  for (int v = lw; v < n_virt; v += NL) {
    const int slot = v % NS;
    if (v >= NS) {
      const int need = Wb * (v / NS);
      while (st_peek(free_lds + slot) < need) __builtin_amdgcn_s_sleep(1);
    }
    const int j0 = (v < n_pre ? v : v - n_pre) * ST_TILE;
    unsigned char* dst = smem + slot * TILEB;
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
#pragma unroll
      for (int q = 0; q < PER_P; ++q) {
        const int c = q * 64 + lane;
        const int i = c / CPR, cp = c % CPR;
        int gi = j0 + i;
        gi = gi < I ? gi : I - 1;
        const T* src = It + p * plane_stride + (long)gi * D + ((cp ^ (i & SWZ)) << 3);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(dst + p * PLANEB + q * 1024), 16, 0, 0);
      }
    }
    v_last = v;
    if (++n_mine > LFL) {
      st_wait_vmcnt<LFL * PER_T>();
      st_wave_fence();
      const int vp = v - LFL * NL;
      *(volatile lds_int*)(full_lds + vp % NS) = vp + 1;
    }
  }
  st_wait_vmcnt<0>();
  st_wave_fence();
  if (v_last >= 0) {
    int vp = v_last - (LFL - 1) * NL;
    if (vp < lw) vp = lw;
    for (; vp <= v_last; vp += NL) *(volatile lds_int*)(full_lds + vp % NS) = vp + 1;
  }
}

// ---- exclusion events (s5_build_events): for a wave's 32 users, one 32-bit word per excluded (user, item) of the scored item range,
// ordered by item tile: tile << 11 | lane that holds the accumulator << 5 | its bit. The wave reads the stream with scalar loads, a quad
// at a time and one quad ahead (w: current, shifted down as events are consumed; n: next), and applies an event with one v_cmp /
// v_cndmask / v_or. Scalar loads do not share a counter with the candidate stores (a per-lane walk of the CSR rows has to wait on
// vmcnt, i.e. for every store in flight), and a user with thousands of exclusions costs its events, not a serialised round per entry
// for the whole wave. The stream is read through the CONSTANT address space: hipcc turns a wave-uniform load from global memory into
// s_load only when it can prove that nothing in the kernel writes there; it could not, used global_load_dwordx4 + VGPRs for the window,
// and the wait for that load — vmcnt(0), i.e. for every candidate store in flight — sat inside the event loop: +0.28 ms per pass.
struct StEvents {
  typedef const __attribute__((address_space(4))) unsigned int* ev_ptr;
  typedef unsigned int ev_quad __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(4))) ev_quad* ev_quad_ptr;
  bool has;                              // wave-uniform
  ev_ptr evp;
  unsigned int w0, w1, w2, w3, n0, n1, n2, n3;
  int ev_rem, ev_q;
  // has: events given and the wave's unit has a group_base entry (a wave past the last user group — padding of the last workgroup — has none)
  __device__ __forceinline__ StEvents(const unsigned int* events, const int* group_base, long unit, bool has_)
      : has(has_), evp(nullptr), w0(S5_EV_NONE), w1(S5_EV_NONE), w2(S5_EV_NONE), w3(S5_EV_NONE), n0(S5_EV_NONE), n1(S5_EV_NONE),
        n2(S5_EV_NONE), n3(S5_EV_NONE), ev_rem(4), ev_q(8) {
    if (has) evp = (ev_ptr)events + ((const __attribute__((address_space(4))) int*)group_base)[unit];
    restart();
  }
  // back to the first event of the stream
  __device__ __forceinline__ void restart() {
    if (has) {
      const ev_quad qa = *(ev_quad_ptr)(evp), qb = *(ev_quad_ptr)(evp + 4);
      w0 = qa.x; w1 = qa.y; w2 = qa.z; w3 = qa.w; n0 = qb.x; n1 = qb.y; n2 = qb.z; n3 = qb.w;
      ev_rem = 4; ev_q = 8;
    }
  }
  // the window moves on by one event (a quad at a time is refilled by a scalar load, one quad ahead)
  __device__ __forceinline__ void next() {
    w0 = w1; w1 = w2; w2 = w3;
    if (--ev_rem == 0) {
      w0 = n0; w1 = n1; w2 = n2; w3 = n3;
      const ev_quad qn = *(ev_quad_ptr)(evp + ev_q);
      n0 = qn.x; n1 = qn.y; n2 = qn.z; n3 = qn.w;
      ev_rem = 4; ev_q += 4;
    }
  }
  // f(event) for every event of tile `tile`, consuming them
  template <typename F>
  __device__ __forceinline__ void for_tile(unsigned int tile, F&& f) {
    if (has) {
      while ((w0 >> 11) == tile) {
        f(w0);
        next();
      }
    }
  }
};

// ---- the consumer side of the ring: FULL / FREE words per slot, the slot of the next tile of the sequence, and `peek` = the FULL word of
// the next slot as read while the current tile was in its MFMAs (stale at worst: slow poll)
template <int NS>
struct StRing {
  lds_int* full;
  lds_int* free;
  int slot_next;
  int peek;
  __device__ __forceinline__ int take() {                  // = V % NS of the next tile V, kept as a wrapping counter
    const int slot = slot_next;
    slot_next = slot + 1 == NS ? 0 : slot + 1;
    return slot;
  }
  // a tile that is not this (partial) wave's: wait for it and release it — the wave stays in step with the ring (a slot may only be
  // released after its tile has been published: the loader counts releases per slot)
  __device__ __forceinline__ void skip(int V) {
    const int slot = take();
    while (st_peek(full + slot) != V + 1) __builtin_amdgcn_s_sleep(1);
    st_wave_fence();
    s5_lds_add_lane0(free + slot, 1);
    peek = 0;
  }
};

// ---- one ring tile through the matrix pipe: wait for tile V, S^T = I x U^T into acc (the first MFMA of a chain takes the inline constant
// 0 as C), release the slot. Fragment reads run PFV steps ahead of the MFMAs that consume them (register ring of PFV + 1 steps); the
// scheduling barriers keep hipcc from sinking the reads back to their use (it otherwise issues read, wait, MFMA in turn and a wave shows
// the LDS latency sixteen times per tile). Fragment f of K step s: row f * 32 + l31 of the slot, 16-byte chunk (2 s + half) ^ (l31 & SWZ)
// = byte offset (s << 5) ^ lxh; lxh is pinned per tile so that the KS offsets are not kept in registers (one v_xad_u32 per read).
template <class Pol, int NS, int PFV>
__device__ __forceinline__ void st_tile_mma(StRing<NS>& ring, const unsigned char* smem, const Pol& pol, int V, int l31, int half,
                                            f32x16 (&acc)[Pol::NJ]) {
  constexpr int KS = Pol::KS, NF = Pol::NF;
  constexpr int ROWB = KS * 16 * 2;
  constexpr int TILEB = Pol::PLANES * 32 * Pol::NJ * ROWB;
  constexpr int SWZ = (KS * 2 >= 16) ? 15 : (KS * 2 - 1);
  typedef typename Pol::Frag Frag;
  const int slot = ring.take();
  if (__builtin_amdgcn_readfirstlane(ring.peek) != V + 1) {
    while (st_peek(ring.full + slot) != V + 1) __builtin_amdgcn_s_sleep(1);
  }
  st_wave_fence();
  Frag bf[PFV + 1][NF];
  const unsigned char* rowp = smem + slot * TILEB + l31 * ROWB;
  unsigned int lxh = (unsigned int)(((l31 & SWZ) << 4) ^ (half << 4));
  asm volatile("" : "+v"(lxh));
#pragma unroll
  for (int s = 0; s < PFV && s < KS; ++s) {
#pragma unroll
    for (int f = 0; f < NF; ++f) bf[s][f] = *reinterpret_cast<const Frag*>(rowp + f * 32 * ROWB + (((unsigned int)s << 5) ^ lxh));
  }
  if constexpr (S5_PRIO != 0) __builtin_amdgcn_s_setprio(S5_PRIO);     // MFMA phase wins the SIMD's issue arbitration
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (s + PFV < KS) {
#pragma unroll
      for (int f = 0; f < NF; ++f)
        bf[(s + PFV) % (PFV + 1)][f] = *reinterpret_cast<const Frag*>(rowp + f * 32 * ROWB + (((unsigned int)(s + PFV) << 5) ^ lxh));
    }
    if (s == KS / 2) ring.peek = *(volatile lds_int*)(ring.full + ring.slot_next);
    __builtin_amdgcn_sched_barrier(0);
    pol.mma(acc, bf[s % (PFV + 1)], s);
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (S5_PRIO != 0) __builtin_amdgcn_s_setprio(0);
  s5_lds_done(acc[0], acc[Pol::NJ - 1]);
  s5_lds_add_lane0(ring.free + slot, 1);
}

// the fp16 operand policy (score_topk_f16_n.hip, pass 1 of score_topk_f16_2p.hip): fp16 user and item rows, one 32x32x16 MFMA per
// accumulator tile and K step
template <int KS_, int NJ_>
struct StF16 {
  static constexpr int KS = KS_, NJ = NJ_, PLANES = 1, NF = NJ_;
  static constexpr int MAXW = S5_MAXW, NL = S5_NL, PRE_TILES = S5_PRE_TILES;
  static constexpr int PF = NJ == 1 ? S5_PF1 : S5_PF2;     // fragment prefetch distance in K steps
  static constexpr int PF_PRE = KS >= 16 ? 1 : PF;         // ... in the prefix pass (D = 256: the class maxima need the registers)
  typedef _Float16 UT;
  typedef _Float16 IT;
  typedef f16x8 Frag;
  f16x8 ufrag[KS];                                         // B operand: user row, k = 16 s + 8 half + j
  __device__ __forceinline__ void load_users(const _Float16* U, long ur, int half) {
    const f16x8* src = reinterpret_cast<const f16x8*>(U + ur * (KS * 16));
#pragma unroll
    for (int s = 0; s < KS; ++s) ufrag[s] = src[2 * s + half];
    // Name the fragments once before the tile loops: hipcc then waits for these loads HERE. Left pending, its wait lands in front of
    // the first MFMA inside the loop as s_waitcnt vmcnt(0) — which, on every later tile, waits for the candidate stores of the
    // previous tile (appends are inline assembly the compiler's counter model does not see).
#pragma unroll
    for (int s = 0; s < KS; ++s) s5_pin8(ufrag[s]);
  }
  __device__ __forceinline__ void mma(f32x16 (&acc)[NJ], const f16x8 (&b)[NF], int s) const {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) acc[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b[nj], ufrag[s], s == 0 ? zero16 : acc[nj], 0, 0, 0);
  }
};

// ---- the one-pass consumer (see the header of score_topk_f16_n.hip). Lane (u, h) holds for ONE user the scores of 16 items of every
// 32-item tile; its threshold and its byte cursor into the user's buffer half h (the thresholds of the two halves of a user are equal).
// WIDE (33 <= k <= 128, chosen on the host): a separate instantiation, the k <= 32 one is compiled from the same text as before.
// A user's 32 class maxima bound the k-th best score only while k <= 32, so the wide form has no prefix pass and no class-maxima
// refresh: its threshold is the exact k-th best score of the user's BUFFERED entries, taken whenever a buffer half passes LIMIT
// (s5_overflow_select_held). That is k distinct, scoreable, already-seen items at or above it, all with smaller indices than any later
// item, so the appends' rule (a > thr) stays valid. It starts at -inf: the first 2 LIMIT / 32 tiles are appended whole and the first
// selection is the bootstrap; with a fixed threshold the k-th of n items lets k / n of the stream through, so every selection
// multiplies the items seen by about 1 + (2 LIMIT - k) / k and a 50k catalogue takes four or five selections per user.
template <class Pol, int NS, bool WIDE = false>
__device__ __forceinline__ void st_one_pass(const typename Pol::UT* U, const typename Pol::IT* It, long Bu, int I, const unsigned int* events,
                                            const int* group_base, int item_offset, int k, int n_pre, int W, int n_part, int P,
                                            int* cnt_out, unsigned long long* gbuf) {
  constexpr int KS = Pol::KS, NJ = Pol::NJ;
  constexpr int D = KS * 16;
  constexpr int ST_TILE = 32 * NJ;
  constexpr int LIMIT = S5_CAPH - 16 * NJ;                 // a tile adds at most 16 NJ entries to a (user, half) buffer
  constexpr int TILEB = Pol::PLANES * ST_TILE * D * 2;
  static_assert(LIMIT >= 32, "k <= 32 entries must fit below the compaction limit");
  // wide lists: a half over LIMIT holds k entries by itself, and the survivors of a selection (at most 64 per half) leave a tile's room
  static_assert(!WIDE || (LIMIT >= 128 && 64 + 16 * NJ <= LIMIT), "k <= 128: survivors split over both halves must leave room below LIMIT");
  constexpr bool CML = KS >= S5_CML_KS;                    // class maxima of the main pass in LDS instead of registers
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  lds_int* full_lds = (lds_int*)(smem + NS * TILEB);
  lds_int* free_lds = full_lds + NS;
  // CML: [consumer wave][16 classes][64 lanes] floats behind the ring and its counters
  const unsigned int cm_addr = (unsigned int)(size_t)(smem + NS * TILEB + 2 * NS * 4 + 16) + (unsigned int)((threadIdx.x >> 6) * 4096 + (threadIdx.x & 63) * 4);

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const StUnit un(Bu, W, n_part, P, wave);
  const int n_tiles = (I + ST_TILE - 1) / ST_TILE;
  const int n_virt = n_pre + n_tiles;                      // tile sequence: prefix tiles 0 .. n_pre - 1, then all tiles

  if (t < NS) { full_lds[t] = 0; free_lds[t] = 0; }
  __syncthreads();                                         // the only workgroup barrier of the kernel

  const int cslots = W + (n_part > 0 ? 1 : 0);             // wave slots in front of the loader waves
  if (wave == W && n_part > 0 && !un.partial) return;      // the slot of the partial wave in a workgroup that has none
  if (wave >= cslots) {
    st_loader<Pol::PLANES, ST_TILE, D, NS, Pol::NL>(smem, full_lds, free_lds, It, I, n_pre, n_virt, un.Wb, wave - cslots, lane);
    return;
  }

  // ------------------------------------------------ consumer waves ------------------------------------------------------
  Pol pol;
  {
    const long r = un.unit * 32 + l31;
    pol.load_users(U, r < Bu ? r : Bu - 1, half);          // rows >= Bu: a copy of the last row (never read back)
  }
  unsigned long long* wgb = gbuf + un.brow0 * (2 * S5_CAPH);      // wave-uniform: buffers of the wave's 32 users
  const i32x4 wrs = s5_block_rsrc(wgb);
  StEvents ev(events, group_base, un.unit, events != nullptr && un.unit < un.n_units);
  StRing<NS> ring{full_lds, free_lds, 0, 0};
  float thr = -INFINITY;
  const int lane_base = (l31 * 2 + half) * S5_CAPH * 8;
  int pos = lane_base;

  // one item tile: MFMAs, then the exclusion events of the tile -> one bit per excluded score in the lane that holds it
  auto tile = [&](int V, int j0, auto pfv, f32x16 (&acc)[NJ], unsigned int& ex, bool& have_ex) {
    st_tile_mma<Pol, NS, decltype(pfv)::value>(ring, smem, pol, V, l31, half, acc);
    ex = 0u;
    have_ex = false;
    ev.for_tile((unsigned int)(j0 / ST_TILE), [&](unsigned int e) {
      ex |= lane == (int)((e >> 5) & 63u) ? 1u << (e & 31u) : 0u;
      have_ex = true;
    });
  };
  auto skip = [&](int V, int j0) {
    ring.skip(V);
    ev.for_tile((unsigned int)(j0 / ST_TILE), [](unsigned int) {});
  };
  // catalogue end inside the tile: padded columns never count (item (r & 3) + 8 (r >> 2) + 32 nj of this lane exists iff < lim)
  auto mask_tail = [&](int j0, f32x16 (&acc)[NJ]) {
    if (j0 + ST_TILE > I) {
      const int lim = I - j0 - 4 * half;
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool in = nj * 32 + (r & 3) + 8 * (r >> 2) < lim;
          acc[nj][r] = in ? acc[nj][r] : -INFINITY;
        }
      }
    }
  };

  // ---- pass 1: prefix tiles, running maximum per accumulator register (item class) ----
  float cm[16];                                            // item class = (lane half, accumulator register): 32 per user
#pragma unroll
  for (int r = 0; r < 16; ++r) cm[r] = -INFINITY;
  if (un.partial) {
    for (int v = 0; v < n_pre; ++v) skip(v, v * ST_TILE);
    ev.restart();
  } else if (!WIDE && n_pre > 0) {
    for (int v = 0; v < n_pre; ++v) {
      const int j0 = v * ST_TILE;
      f32x16 acc[NJ];
      unsigned int ex;
      bool have_ex;
      tile(v, j0, std::integral_constant<int, Pol::PF_PRE>(), acc, ex, have_ex);
      if (have_ex) {                                       // excluded scores must not raise a class maximum
        const unsigned int ex0 = ex;
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[nj][r] = ((ex0 >> (nj * 16 + r)) & 1u) ? -INFINITY : acc[nj][r];
        }
      }
      mask_tail(j0, acc);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr (NJ == 2) cm[r] = __builtin_fmaxf(cm[r], __builtin_fmaxf(acc[0][r], acc[1][r]));      // one v_max3
        else cm[r] = fmaxf(cm[r], acc[0][r]);
      }
    }
    // k-th largest of the user's 32 class maxima (16 in each of its two lanes), every lane pair for its own user. The threshold
    // admits scores EQUAL to the bound (its items are not in any buffer: the main pass meets them again): one ulp below it.
    {
      const float tk = s5_kth_of_32(cm, k);
      const unsigned int key = st_f2key(tk);
      // key 0x007FFFFF is -inf (fewer than k finite classes): no bound. One step below +0.0 in KEY order is -0.0, which the float
      // compare of the appends treats as EQUAL to +0.0 (a > -0.0 is false for a = +0.0: a user whose scores are all exactly zero got an
      // empty list in round 3) — the value below both zeros is the negative denormal -1.4e-45
      unsigned int below = key - 1u;
      below = below == 0x7FFFFFFFu ? 0x7FFFFFFEu : below;
      thr = key > 0x007FFFFFu ? st_key2f(below) : -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) cm[r] = -INFINITY;       // the main pass keeps the class maxima of what it APPENDS
    ev.restart();                                          // the main pass starts again from the first tile
  }
  if constexpr (CML) {
#pragma unroll
    for (int r = 0; r < 16; ++r) *(__attribute__((address_space(3))) float*)(size_t)(cm_addr + r * 256) = -INFINITY;
  }

  // ---- pass 2: all tiles, lane-local threshold filter and appends ----
  const int pos_limit = lane_base + LIMIT * 8;
  // threshold refresh from the class maxima: after tiles 0, 1, 2, 3, 5, 8, 12, ... (gaps growing by half) while the thresholds are
  // still crude, every S5_RF tiles in the steady state
  int next_rf = (n_pre > 0 && !un.partial) ? S5_RF - 1 : 0;
  int part_next = un.part;                                 // next tile of this part (a full wave: every tile)
  for (int tl = 0; tl < n_tiles; ++tl) {
    if (tl != part_next) {                                 // (partial waves only) another part's tile
      skip(n_pre + tl, tl * ST_TILE);
      continue;
    }
    part_next += un.n_parts;
    if (__ballot(pos > pos_limit)) {
      // ---- overflow (cold): a (user, half) buffer is nearly full — select that user's k best so that this tile's appends fit
      unsigned long long need = __ballot(pos > pos_limit);
      need = (need | (need >> 32)) & 0xFFFFFFFFull;
      const int cnt = (pos - lane_base) >> 3;
      while (need) {
        const int u = __ffsll((long long)need) - 1;
        need &= need - 1ull;
        const int c0 = __builtin_amdgcn_readlane(cnt, u), c1 = __builtin_amdgcn_readlane(cnt, u + 32);
        unsigned long long* b0 = wgb + (long)u * (2 * S5_CAPH);
        float nt;
        if constexpr (WIDE) nt = s5_overflow_select_held(b0, b0 + S5_CAPH, c0, c1, k, lane);
        else nt = s5_overflow_select(b0, b0 + S5_CAPH, c0, c1, k, lane);
        if (c0 + c1 >= k && l31 == u) {
          thr = nt > thr ? nt : thr;
          pos = lane_base + (half ? (k >> 1) : k - (k >> 1)) * 8;
        }
      }
    }
    const int j0 = tl * ST_TILE;
    f32x16 acc[NJ];
    unsigned int ex;
    bool have_ex;
    tile(n_pre + tl, j0, std::integral_constant<int, Pol::PF>(), acc, ex, have_ex);
    mask_tail(j0, acc);
    const unsigned int item_lane = 0xFFFFFFFFu - (unsigned int)(item_offset + j0 + 4 * half);
    // Threshold ladder. A wave is in-order and a vector -> scalar hand-over (v_cmp -> s_cbranch, v_cmp -> s_and_saveexec) costs
    // ~25 cycles every time, so the ladder does ALL its vector work first — the maximum of every PAIR of accumulator registers
    // and one v_cmp per pair into its own SGPR pair, back to back — then dispatches on scalar registers only (one branch for
    // "nothing in this tile", s_cmp + branch per pair), and a pair that fired runs a branch-free append per register in which
    // the vector ALU writes EXEC itself (s5_try_append).
    unsigned long long gm[8 * NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
#pragma unroll
      for (int g = 0; g < 8; ++g) gm[nj * 8 + g] = __ballot(s5_max2(acc[nj][2 * g], acc[nj][2 * g + 1]) > thr);
    }
    unsigned long long any_g = 0ull;
#pragma unroll
    for (int i = 0; i < 8 * NJ; ++i) any_g |= gm[i];
    if (any_g) {
      // item of register r: nj * 32 + (r & 3) + 8 * (r >> 2) (+ 4 * half, in item_lane); exclusion bit nj * 16 + r. A pair that
      // did not fire is the common case: its test falls through (the append blocks are laid out of line: a taken branch costs the
      // wave an instruction-fetch bubble, sixteen of them per tile)
#define ST_PAIR(NJI, G)                                                                                                  \
      if (__builtin_expect(gm[(NJI) * 8 + (G)] != 0ull, 0)) {                                                            \
        s5_try_append<(1u << ((NJI) * 16 + 2 * (G))), (NJI) * 32 + ((2 * (G)) & 3) + 8 * ((2 * (G)) >> 2), true, CML, 2 * (G)>(acc[NJI][2 * (G)], thr, ex, pos, item_lane, wrs, cm[2 * (G)], cm_addr);             \
        s5_try_append<(1u << ((NJI) * 16 + 2 * (G) + 1)), (NJI) * 32 + ((2 * (G) + 1) & 3) + 8 * ((2 * (G) + 1) >> 2), true, CML, 2 * (G) + 1>(acc[NJI][2 * (G) + 1], thr, ex, pos, item_lane, wrs, cm[2 * (G) + 1], cm_addr); \
      }
      ST_PAIR(0, 0) ST_PAIR(0, 1) ST_PAIR(0, 2) ST_PAIR(0, 3) ST_PAIR(0, 4) ST_PAIR(0, 5) ST_PAIR(0, 6) ST_PAIR(0, 7)
      if constexpr (NJ == 2) {
        ST_PAIR(NJ - 1, 0) ST_PAIR(NJ - 1, 1) ST_PAIR(NJ - 1, 2) ST_PAIR(NJ - 1, 3) ST_PAIR(NJ - 1, 4) ST_PAIR(NJ - 1, 5) ST_PAIR(NJ - 1, 6) ST_PAIR(NJ - 1, 7)
      }
#undef ST_PAIR
    }
    if (!WIDE && tl >= next_rf) {
      // every later item has a larger index than the k buffered items at or above the bound: it needs a strictly larger score
      if constexpr (CML) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's ds_max updates have been performed
#pragma unroll
        for (int r = 0; r < 16; ++r) cm[r] = *(volatile __attribute__((address_space(3))) float*)(size_t)(cm_addr + r * 256);
      }
      const float tk = s5_kth_of_32(cm, k);
      thr = tk > thr ? tk : thr;
      const int gap = (tl + 2) >> 1;
      next_rf = tl + (gap < S5_RF ? gap : S5_RF);
    }
  }
  // fill counts and final thresholds of the wave's 64 buffer halves: the final selection + ranking is score_topk_finalize_kernel's
  {
    int2 o;
    o.x = (pos - lane_base) >> 3;
    o.y = (int)__float_as_uint(thr);
    reinterpret_cast<int2*>(cnt_out)[(un.brow0 + l31) * 2 + half] = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: one launch path for both one-pass routes
// ---------------------------------------------------------------------------------------------------------------------------------
// final selection of the one-pass kernels' candidate buffers (s5_finalize, score_topk_cand.h); defined in score_topk_f16_n.hip
__global__ void score_topk_finalize_kernel(long Bu, int k, long n_full_units, int P, const int* __restrict__ cnt,
                                           const unsigned long long* __restrict__ gbuf, float* __restrict__ out_val, int* __restrict__ out_idx);
// ... of the wide instantiations (33 <= k <= 128)
__global__ void score_topk_rank_wide_kernel(long Bu, int k, long n_full_units, int P, const int* __restrict__ cnt,
                                            const unsigned long long* __restrict__ gbuf, float* __restrict__ out_val, int* __restrict__ out_idx);

// whole units + the last workgroup's padding + one row group per partial wave
static long st_padded_users(long Bu, int maxw) { return sbr_cdiv(Bu, 32) * 32 + 32L * maxw + 32L * s5_n_cu(); }
// candidate buffers + fill counts / final thresholds
static long st_workspace_bytes(long Bu, int maxw) {
  const long padded = st_padded_users(Bu, maxw);
  return padded * 2 * S5_CAPH * 8 + s5_al16(padded * 2 * 8);
}

// kern: the route's instantiation of its one-pass kernel (the st_one_pass signature with the route's operand types); what: the C entry,
// for messages
template <class Pol, int NS, bool WIDE = false, typename UT, typename IT>
static int st_launch(void (*kern)(const UT*, const IT*, long, int, const unsigned int*, const int*, int, int, int, int, int, int, int*, unsigned long long*),
                     const char* what, const UT* U, const IT* It, long Bu, int I, const long* u_idx, const long* eptr, const int* eidx,
                     long excl_nnz, int item_offset, int k, float* out_val, int* out_idx, void* workspace, long workspace_bytes, void* ev_buf,
                     long ev_bytes, int build_events, hipStream_t s) {
  constexpr int NJ = Pol::NJ;
  const S5Plan plan = s5_plan(Bu, Pol::MAXW);
  const int W = plan.W;
  const long n_wg = plan.n_wg;
  const long padded = st_padded_users(Bu, Pol::MAXW);
  const long buf_bytes = padded * 2 * S5_CAPH * 8;
  SBR_REQUIRE(W + (plan.n_part > 0 ? 1 : 0) <= Pol::MAXW, "%s: internal: wave count", what);
  SBR_REQUIRE(n_wg * 32L * W + 32L * plan.n_part <= padded && sbr_cdiv(Bu, 32) * 32 + 32L * plan.n_part <= padded, "%s: internal: padding", what);
  SBR_REQUIRE(workspace && workspace_bytes >= st_workspace_bytes(Bu, Pol::MAXW), "%s: workspace of %ld bytes needed (%s_workspace), %ld given",
              what, st_workspace_bytes(Bu, Pol::MAXW), what, workspace_bytes);
  int* cnt = (int*)((char*)workspace + buf_bytes);
  const bool with_excl = eptr != nullptr && excl_nnz > 0;
  S5Events evs = {nullptr, nullptr};
  if (with_excl) {
    const int rc = s5_build_events(ev_buf, ev_bytes, Bu, I, u_idx, eptr, eidx, excl_nnz, item_offset, 32 * NJ, build_events != 0, &evs, s);
    if (rc) return rc;
  }
  // the ring and its counters (+ the class maxima of D = 256)
  const size_t lds = (size_t)NS * Pol::PLANES * (32 * NJ) * Pol::KS * 32 + 2 * NS * 4 + 16 + (Pol::KS >= S5_CML_KS ? (size_t)Pol::MAXW * 4096 : 0);
  SBR_REQUIRE(lds <= 160 * 1024, "%s: LDS budget exceeded (%zu bytes)", what, lds);
  // prefix pass (class maxima only, no appends) over the first PRE_TILES tiles: its bound spares the main pass the appends of its first
  // tiles (every score passes a threshold of -inf), at the price of scoring those tiles twice (fp16 route, measured on c2: 0 tiles
  // 1.76 ms, 8: 1.59, 16: 1.54, 32: 1.55, 65: 1.58)
  const int n_tiles = sbr_cdiv(I, 32 * NJ);
  const int n_pre = !WIDE && n_tiles >= 6 * Pol::PRE_TILES ? Pol::PRE_TILES : 0;      // (wide lists bootstrap from their first selection)
  static SbrLdsSlot lds_slot;                                      // (one per instantiation, each of which launches one kernel)
  const int lds_rc = sbr_raise_lds(what, (const void*)kern, &lds_slot, lds);
  if (lds_rc) return lds_rc;
  // (a full wave of the last workgroups may own a unit past the last user: it scores a copy of the last user and nobody reads its buffers)
  kern<<<(unsigned int)n_wg, (W + (plan.n_part > 0 ? 1 : 0) + Pol::NL) * 64, lds, s>>>(U, It, Bu, I, evs.events, evs.group_base, item_offset, k,
                                                                                      n_pre, W, plan.n_part, plan.P, cnt, (unsigned long long*)workspace);
  SBR_CHECK_LAUNCH(what);
  char fin[64];
  snprintf(fin, sizeof fin, "%s (final selection)", what);
  (WIDE ? score_topk_rank_wide_kernel : score_topk_finalize_kernel)<<<(unsigned int)sbr_cdiv(Bu, 4), 256, 0, s>>>(
      Bu, k, plan.n_part > 0 ? (long)n_wg * W : (1L << 40), plan.P, cnt, (const unsigned long long*)workspace, out_val, out_idx);
  SBR_CHECK_LAUNCH(fin);
  return SBR_OK;
}
