// Candidate buffers of the one-pass fused scorers (score_topk_f16_n.hip: fp16 operands; score_topk_f32s.hip: fp32 operands on the
// bf16 pipe over exact three-way splits): the raw-entry append, the overflow selection of a full (user, half) buffer and the final
// selection + ranking. Both kernels fill the same buffer layout, so one copy of each piece serves both. Device code only (each
// translation unit compiles its own copy).
#pragma once
#include "score_topk_shared.h"

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

#ifndef S5_CAPH
#define S5_CAPH 256                      // candidate entries per (user, lane half); multiple of 64
#endif
#define S5_EH (S5_CAPH / 64)             // entries of one buffer half per lane when a wave holds a whole user's buffers

// All 64 lanes: the scorer's OVERFLOW path (a (user, half) buffer ran full: ties at the threshold, or a threshold that cannot rise).
// The k best of the n0 + n1 raw entries of a user's two buffer halves are found by a bitwise binary search for the k-th largest
// composite key (score key << 32 | ~item: ties at the k-th score keep the smallest item indices) over ballot counts; written for few
// registers instead of speed — the entries are re-read from the buffers in every round of the search instead of being held in
// 2 x S5_EH register pairs per lane, which would cost the hot loop its fourth wave per SIMD. Survivors go back split over both
// halves (k - k / 2 and k / 2: both keep room). Returns the k-th best score; -inf (nothing moved) below k entries.
__device__ __forceinline__ float s5_overflow_select(unsigned long long* b0, unsigned long long* b1, int n0_any, int n1_any, int k, int lane) {
  const int n0 = __builtin_amdgcn_readfirstlane(n0_any), n1 = __builtin_amdgcn_readfirstlane(n1_any);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // written and read by this wave only
  if (n0 + n1 < k) return -INFINITY;
  const int c0 = (n0 + 63) >> 6, c1 = (n1 + 63) >> 6;
  auto raw_at = [&](bool first, int j) -> unsigned long long {
    const int q = lane + 64 * j;
    return q < (first ? n0 : n1) ? (first ? b0 : b1)[q] : 0ull;
  };
  auto key_of = [&](unsigned long long raw) -> unsigned long long {     // 0 for an empty slot (raw entries are never 0: ~item != 0)
    return raw ? (((unsigned long long)st_f2key(__uint_as_float((unsigned int)(raw >> 32))) << 32) | (raw & 0xFFFFFFFFull)) : 0ull;
  };
  auto count_ge = [&](unsigned long long C) {
    int cnt = 0;
    for (int j = 0; j < c0; ++j) cnt += __popcll(__ballot(key_of(raw_at(true, j)) >= C));
    for (int j = 0; j < c1; ++j) cnt += __popcll(__ballot(key_of(raw_at(false, j)) >= C));
    return cnt;
  };
  unsigned int T = 0u;
  int c_ge = n0 + n1;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned int trial = T | (1u << bit);
    const int cnt = count_ge((unsigned long long)trial << 32);
    if (cnt >= k) { T = trial; c_ge = cnt; if (cnt == k) break; }
  }
  unsigned long long C = (unsigned long long)T << 32;
  if (c_ge != k) {
    unsigned int Lw = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned int trial = Lw | (1u << bit);
      Lw = count_ge(((unsigned long long)T << 32) | trial) >= k ? trial : Lw;
    }
    C |= (unsigned long long)Lw;
  }
  // survivors land in entries [0, 32) of the two halves: chunk 0 of both is taken into registers first, the other chunks are
  // streamed (read, keep, store), chunk 0's survivors go last
  const unsigned long long r00 = raw_at(true, 0), r10 = raw_at(false, 0);
  const int kh = k - (k >> 1);
  int before = 0;
  auto place = [&](unsigned long long raw) {
    const bool keep = key_of(raw) >= C;
    const unsigned long long m = __ballot(keep);
    const int p = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (keep) (p < kh ? b0 + p : b1 + (p - kh))[0] = raw;
    before += __popcll(m);
  };
  for (int j = 1; j < c0; ++j) place(raw_at(true, j));
  for (int j = 1; j < c1; ++j) place(raw_at(false, j));
  place(r00);
  place(r10);
  const float t = st_key2f(T);
  return t == t ? t : -INFINITY;
}

// The same selection for the WIDE instantiations (33 <= k <= 128), where it is the steady mechanism and not a rare event: the appends'
// threshold of a wide list is the exact k-th best score of the user's buffered entries, renewed whenever a buffer half passes the
// limit (a user's 32 class maxima bound nothing beyond k = 32). The user's entries are read ONCE (2 x S5_EH raw entries per lane:
// the accumulators are dead at this point of the tile loop, so the registers are there) and the search runs on registers: up to 32
// rounds over the 32-bit score keys, and 32 more over the item words only when the k-th score is tied. Same result, same survivor
// layout and same return value as s5_overflow_select.
__device__ __forceinline__ float s5_overflow_select_held(unsigned long long* b0, unsigned long long* b1, int n0_any, int n1_any, int k, int lane) {
  const int n0 = __builtin_amdgcn_readfirstlane(n0_any), n1 = __builtin_amdgcn_readfirstlane(n1_any);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // written and read by this wave only
  if (n0 + n1 < k) return -INFINITY;
  unsigned long long raw[2 * S5_EH];
#pragma unroll
  for (int j = 0; j < 2 * S5_EH; ++j) {
    const int hh = j / S5_EH, q = (j % S5_EH) * 64 + lane;
    raw[j] = q < (hh ? n1 : n0) ? (hh ? b1 : b0)[q] : 0ull;
  }
  unsigned int sk[2 * S5_EH];                                // score key; 0 for an empty slot (no trial value is 0)
#pragma unroll
  for (int j = 0; j < 2 * S5_EH; ++j) sk[j] = raw[j] ? st_f2key(__uint_as_float((unsigned int)(raw[j] >> 32))) : 0u;
  unsigned int T = 0u;
  int c_ge = n0 + n1;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned int trial = T | (1u << bit);
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 2 * S5_EH; ++j) cnt += __popcll(__ballot(sk[j] >= trial));
    if (cnt >= k) { T = trial; c_ge = cnt; if (cnt == k) break; }
  }
  unsigned int Lw = 0u;                                      // ties at the k-th score keep the smallest item indices (largest ~item)
  if (c_ge != k) {
    int above = 0;
#pragma unroll
    for (int j = 0; j < 2 * S5_EH; ++j) above += __popcll(__ballot(sk[j] > T));
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned int trial = Lw | (1u << bit);
      int cnt = above;
#pragma unroll
      for (int j = 0; j < 2 * S5_EH; ++j) cnt += __popcll(__ballot(sk[j] == T && (unsigned int)raw[j] >= trial));
      Lw = cnt >= k ? trial : Lw;
    }
  }
  const int kh = k - (k >> 1);
  int before = 0;
#pragma unroll
  for (int j = 0; j < 2 * S5_EH; ++j) {                      // every entry is in registers: the survivors may land anywhere
    const bool keep = sk[j] > T || (sk[j] == T && sk[j] != 0u && (unsigned int)raw[j] >= Lw);
    const unsigned long long m = __ballot(keep);
    const int p = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (keep && p < k) (p < kh ? b0 + p : b1 + (p - kh))[0] = raw[j];
    before += __popcll(m);
  }
  const float t = st_key2f(T);
  return t == t ? t : -INFINITY;
}

// append of one raw candidate entry at byte offset `pos` of the wave's buffer block (`block`: wave-uniform, so the descriptor is
// four SGPRs the compiler builds once per kernel): buffer_store_dwordx2 v[ent], v[pos], s[rsrc], 0 offen
__device__ __forceinline__ void s5_append(unsigned long long* block, int pos, u32x2 ent) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(block, 0, 32 * 2 * S5_CAPH * 8, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b64(ent, rs, pos, 0, 0);
}

// Branch-free append of one accumulator value: lanes with a > thr whose exclusion bit is clear store the raw entry
// (~item = il - C, score bits) at their byte cursor and advance it. The vector ALU writes EXEC itself (v_cmpx), so the
// sequence has no vector -> scalar hand-over and no branch; all lanes are active on entry and on exit. rs: buffer descriptor of
// the wave's candidate block (s5_block_rsrc).
#define S5_STORE_ASM "buffer_store_dword %[tmp], %[pos], %[rs], 0 offen\n\t" "buffer_store_dword %[a], %[pos], %[rs], 0 offen offset:4\n\t"
// CML (D = 256: the user fragments alone take 64 registers): the class maxima live in LDS ([register][lane] floats per wave, the lane's
// slot of class r at cm_addr + 256 r) and the append updates them with a no-return ds_max_f32 under the same EXEC mask.
template <unsigned int BIT, int C, bool EX, bool CML, int R>
__device__ __forceinline__ void s5_try_append(float a, float thr, unsigned int ex, int& pos, unsigned int il, i32x4 rs, float& cmax,
                                              unsigned int cm_addr) {
  unsigned int tmp;
  if constexpr (CML) {
    asm volatile(
        "v_cmpx_gt_f32_e32 %[a], %[thr]\n\t"
        "v_and_b32_e32 %[tmp], %[bit], %[ex]\n\t"
        "v_cmpx_eq_u32_e32 0, %[tmp]\n\t"
        "v_subrev_u32_e32 %[tmp], %[c], %[il]\n\t"
        S5_STORE_ASM
        "v_add_u32_e32 %[pos], 8, %[pos]\n\t"
        "ds_max_f32 %[cma], %[a] offset:%[off]\n\t"
        "s_mov_b64 exec, -1"
        : [pos] "+v"(pos), [tmp] "=&v"(tmp)
        : [a] "v"(a), [thr] "v"(thr), [ex] "v"(ex), [il] "v"(il), [rs] "s"(rs), [bit] "n"(BIT), [c] "n"(C), [cma] "v"(cm_addr), [off] "n"(R * 256)
        : "vcc", "memory");
    return;
  }
  if constexpr (!EX) {                                       // a tile without exclusion events: no exclusion bit to test
    asm volatile(
        "v_cmpx_gt_f32_e32 %[a], %[thr]\n\t"
        "v_subrev_u32_e32 %[tmp], %[c], %[il]\n\t"
        S5_STORE_ASM
        "v_add_u32_e32 %[pos], 8, %[pos]\n\t"
        "v_max_f32_e32 %[cm], %[cm], %[a]\n\t"
        "s_mov_b64 exec, -1"
        : [pos] "+v"(pos), [tmp] "=&v"(tmp), [cm] "+v"(cmax)
        : [a] "v"(a), [thr] "v"(thr), [il] "v"(il), [rs] "s"(rs), [c] "n"(C)
        : "vcc", "memory");
    return;
  }
  asm volatile(
      "v_cmpx_gt_f32_e32 %[a], %[thr]\n\t"
      "v_and_b32_e32 %[tmp], %[bit], %[ex]\n\t"
      "v_cmpx_eq_u32_e32 0, %[tmp]\n\t"
      "v_subrev_u32_e32 %[tmp], %[c], %[il]\n\t"
      S5_STORE_ASM
      "v_add_u32_e32 %[pos], 8, %[pos]\n\t"
      "v_max_f32_e32 %[cm], %[cm], %[a]\n\t"               /* class maximum of what was appended (same EXEC mask) */
      "s_mov_b64 exec, -1"
      : [pos] "+v"(pos), [tmp] "=&v"(tmp), [cm] "+v"(cmax)
      : [a] "v"(a), [thr] "v"(thr), [ex] "v"(ex), [il] "v"(il), [rs] "s"(rs), [bit] "n"(BIT), [c] "n"(C)
      : "vcc", "memory");
}
// raw buffer descriptor of a wave's candidate block: base, stride 0, 32 users x 2 halves x S5_CAPH entries of 8 bytes, gfx950 format word
__device__ __forceinline__ i32x4 s5_block_rsrc(const void* block) {
  const unsigned long long b = (unsigned long long)block;
  i32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned int)b);
  r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned int)(b >> 32) & 0xFFFF);
  r[2] = 32 * 2 * S5_CAPH * 8;
  r[3] = 0x00020000;
  return r;
}

// ---- final selection: one wave per user, four users per workgroup. A user's candidates sit in ONE pair of buffer halves (its unit
// was scored by a full wave) or in P pairs (a remainder unit cut into P parts by item tile, see the scorer). Only candidates at or
// above the largest of the sources' final thresholds can be among the k best (k buffered items lie at or above each): they are
// filtered first (~25 of ~110), gathered into one entry per lane through LDS, ranked by counting (score desc, item index asc) and the
// lanes of rank < k write the output. More than 64 survivors (ties at the threshold, a threshold that never rose): a bitwise binary
// search over ballot counts (entries re-read per round: cold) finds the k-th largest composite key first and exactly k survive.
// Empty slots (-inf, -1) behind fewer than k candidates.
// WIDE (33 <= k <= 128): the appends' threshold is the k-th best score at the user's LAST overflow selection, so nearly everything
// buffered since passes the filter (up to 2 x 240 entries of a full wave's user) — the staging area takes 512 survivors, the k best of
// them are cut out by the register search and ranked two per lane.
template <bool WIDE>
__device__ __forceinline__ void s5_finalize(long Bu, int k, long n_full_units, int P, const int* __restrict__ cnt,
                                            const unsigned long long* __restrict__ gbuf, float* __restrict__ out_val,
                                            int* __restrict__ out_idx) {
  constexpr int CAP = WIDE ? 512 : 256;                      // survivors a wave can stage in LDS
  __shared__ unsigned long long stage[4][CAP];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long ur = (long)blockIdx.x * 4 + w;
  if (ur >= Bu) return;                                      // wave-uniform
  const long unit = ur >> 5, n_units = (Bu + 31) >> 5;
  const int n_src = unit < n_full_units ? 1 : P;
  const long row_first = unit < n_full_units ? ur : n_units * 32 + (unit - n_full_units) * P * 32 + (ur & 31);      // + 32 per part
  auto key_of = [&](unsigned long long raw) -> unsigned long long {     // 0 for an empty slot (raw entries are never 0: ~item != 0)
    return raw ? (((unsigned long long)st_f2key(__uint_as_float((unsigned int)(raw >> 32))) << 32) | (raw & 0xFFFFFFFFull)) : 0ull;
  };
  const int4 c_first = reinterpret_cast<const int4*>(cnt)[row_first];
  float thr = __uint_as_float((unsigned int)__builtin_amdgcn_readfirstlane(c_first.y));
  // every (source, half, 64-entry chunk) in a fixed order; f(raw entry of this lane or 0). The loads of a source are issued together.
  auto for_chunks = [&](auto&& f) {
    for (int sidx = 0; sidx < n_src; ++sidx) {
      const long row = row_first + 32L * sidx;
      const int4 c = sidx == 0 ? c_first : reinterpret_cast<const int4*>(cnt)[row];       // (n0, thr bits, n1, thr bits)
      const int n0 = __builtin_amdgcn_readfirstlane(c.x), n1 = __builtin_amdgcn_readfirstlane(c.z);
      const unsigned long long* b0 = gbuf + row * (2 * S5_CAPH);
      unsigned long long raw[2 * S5_EH];
#pragma unroll
      for (int j = 0; j < 2 * S5_EH; ++j) {
        const int hh = j / S5_EH, q = (j % S5_EH) * 64 + lane;
        raw[j] = q < (hh ? n1 : n0) ? b0[hh * S5_CAPH + q] : 0ull;
      }
#pragma unroll
      for (int j = 0; j < 2 * S5_EH; ++j) {
        if ((j % S5_EH) * 64 < (j / S5_EH ? n1 : n0)) f(raw[j]);                  // wave-uniform
      }
    }
  };
  for (int sidx = 1; sidx < n_src; ++sidx) {
    const float t = __uint_as_float((unsigned int)__builtin_amdgcn_readfirstlane(cnt[(row_first + 32L * sidx) * 4 + 1]));
    thr = t > thr ? t : thr;
  }
  // ---- gather the candidates at or above the threshold, one per lane
  unsigned long long cut = 0ull;                             // survivors: composite key >= cut (when the filter lets too many through)
  int n = 0;
  auto gather = [&](unsigned long long raw) {
    const bool keep = raw != 0ull && (cut ? key_of(raw) >= cut : __uint_as_float((unsigned int)(raw >> 32)) >= thr);
    const unsigned long long m = __ballot(keep);
    const int p = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (keep && p < CAP) stage[w][p] = raw;
    n += __popcll(m);
  };
  for_chunks(gather);
  if (n > CAP) {                                             // cold: exactly k survive a cut at the k-th largest composite key
    auto count_ge = [&](unsigned long long C) {
      int cn = 0;
      for_chunks([&](unsigned long long raw) { cn += __popcll(__ballot(key_of(raw) >= C && raw != 0ull)); });
      return cn;
    };
    unsigned int T = 0u;
    int c_ge = 1 << 30;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned int trial = T | (1u << bit);
      const int cn = count_ge((unsigned long long)trial << 32);
      if (cn >= k) { T = trial; c_ge = cn; if (cn == k) break; }
    }
    cut = (unsigned long long)T << 32;
    if (c_ge != k) {
      unsigned int Lw = 0u;
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned int trial = Lw | (1u << bit);
        Lw = count_ge(((unsigned long long)T << 32) | trial) >= k ? trial : Lw;
      }
      cut |= (unsigned long long)Lw;
    }
    st_wave_fence();
    n = 0;
    for_chunks(gather);
  }
  st_wave_fence();                                           // LDS operations of a wave execute in order
  if constexpr (WIDE) {
    // up to CAP survivors, CAP / 64 per lane as composite keys; more than 128 of them: exactly k survive the cut at the k-th largest key
    unsigned long long e8[CAP / 64];
#pragma unroll
    for (int q = 0; q < CAP / 64; ++q) e8[q] = key_of(q * 64 + lane < n ? stage[w][q * 64 + lane] : 0ull);
    unsigned long long kcut = 0ull;
    if (n > 128) {
      auto count_ge = [&](unsigned long long C) {
        int cn = 0;
#pragma unroll
        for (int q = 0; q < CAP / 64; ++q) cn += __popcll(__ballot(e8[q] >= C));
        return cn;
      };
      unsigned int T = 0u;
      int c_ge = 1 << 30;
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned int trial = T | (1u << bit);
        const int cn = count_ge((unsigned long long)trial << 32);
        if (cn >= k) { T = trial; c_ge = cn; if (cn == k) break; }
      }
      kcut = (unsigned long long)T << 32;
      if (c_ge != k) {
        unsigned int Lw = 0u;
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned int trial = Lw | (1u << bit);
          Lw = count_ge(((unsigned long long)T << 32) | trial) >= k ? trial : Lw;
        }
        kcut |= (unsigned long long)Lw;
      }
    }
    st_wave_fence();
    n = 0;
#pragma unroll
    for (int q = 0; q < CAP / 64; ++q) {
      const bool keep = e8[q] >= kcut && e8[q] != 0ull;
      const unsigned long long m = __ballot(keep);
      const int p = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
      if (keep && p < 128) stage[w][p] = e8[q];
      n += __popcll(m);
    }
    n = n < 128 ? n : 128;
    st_wave_fence();
    // two survivors per lane, ranked by counting (composite keys are distinct: rank = number of larger keys)
    const unsigned long long ea = lane < n ? stage[w][lane] : 0ull, eb = lane + 64 < n ? stage[w][lane + 64] : 0ull;
    int ra = 0, rb = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned long long kj = stage[w][j];             // wave-uniform address: an LDS broadcast
      ra += kj > ea;
      rb += kj > eb;
    }
    if (lane < n && ra < k) {
      out_val[ur * k + ra] = st_key2f((unsigned int)(ea >> 32));
      out_idx[ur * k + ra] = (int)(0xFFFFFFFFu - (unsigned int)(ea & 0xFFFFFFFFull));
    }
    if (lane + 64 < n && rb < k) {
      out_val[ur * k + rb] = st_key2f((unsigned int)(eb >> 32));
      out_idx[ur * k + rb] = (int)(0xFFFFFFFFu - (unsigned int)(eb & 0xFFFFFFFFull));
    }
    const int nkw = n < k ? n : k;
#pragma unroll
    for (int p = lane; p < 128; p += 64) {                   // fewer than k candidates: empty slots behind them, positions >= 64 included
      if (p >= nkw && p < k) {
        out_val[ur * k + p] = -INFINITY;
        out_idx[ur * k + p] = -1;
      }
    }
    return;
  }
  unsigned long long e;
  if (n <= 64) {
    e = key_of(lane < n ? stage[w][lane] : 0ull);
  } else {
    // 65 .. CAP survivors (a user of a remainder unit: the parts' thresholds are those of a quarter of the catalogue each): the same
    // search for the k-th largest composite key, over registers
    unsigned long long e4[CAP / 64];
#pragma unroll
    for (int q = 0; q < CAP / 64; ++q) e4[q] = key_of(q * 64 + lane < n ? stage[w][q * 64 + lane] : 0ull);
    auto count_ge = [&](unsigned long long C) {
      int cn = 0;
#pragma unroll
      for (int q = 0; q < CAP / 64; ++q) cn += __popcll(__ballot(e4[q] >= C));
      return cn;
    };
    unsigned int T = 0u;
    int c_ge = 1 << 30;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned int trial = T | (1u << bit);
      const int cn = count_ge((unsigned long long)trial << 32);
      if (cn >= k) { T = trial; c_ge = cn; if (cn == k) break; }
    }
    unsigned long long kcut = (unsigned long long)T << 32;
    if (c_ge != k) {
      unsigned int Lw = 0u;
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned int trial = Lw | (1u << bit);
        Lw = count_ge(((unsigned long long)T << 32) | trial) >= k ? trial : Lw;
      }
      kcut |= (unsigned long long)Lw;
    }
    st_wave_fence();
    n = 0;
#pragma unroll
    for (int q = 0; q < CAP / 64; ++q) {
      const bool keep = e4[q] >= kcut && e4[q] != 0ull;
      const unsigned long long m = __ballot(keep);
      const int p = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
      if (keep && p < 64) stage[w][p] = e4[q];
      n += __popcll(m);
    }
    st_wave_fence();
    e = lane < n ? stage[w][lane] : 0ull;
  }
  const int h32 = (int)(e >> 32), l32 = (int)e;
  int rk = 0;
  for (int j = 0; j < n; ++j) {
    const unsigned long long kj = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(h32, j) << 32) |
                                  (unsigned long long)(unsigned int)__builtin_amdgcn_readlane(l32, j);
    rk += kj > e;
  }
  const int nk = n < k ? n : k;
  if (lane < n && rk < k) {
    out_val[ur * k + rk] = st_key2f((unsigned int)(e >> 32));
    out_idx[ur * k + rk] = (int)(0xFFFFFFFFu - (unsigned int)(e & 0xFFFFFFFFull));
  }
  if (lane >= nk && lane < k) {                              // fewer than k candidates: empty slots behind them
    out_val[ur * k + lane] = -INFINITY;
    out_idx[ur * k + lane] = -1;
  }
}
