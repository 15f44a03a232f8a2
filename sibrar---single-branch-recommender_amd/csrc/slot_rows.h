// Code shared by the losses over one positive and many sampled negatives per batch row (ultragcn.hip, simplex.hip): the chunk loads of
// a lane group, the group's geometry (the one host function here: the entries' dispatch needs it), and the device walk of one table
// row's slots behind a stable sort of the slots' keys.
#pragma once
#include "common.h"

// V columns of a row at once: 4 (one 16-byte access) when D % 4 == 0, else 1.
template <int V> struct SbrRowChunk;
template <> struct SbrRowChunk<4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct SbrRowChunk<1> {
  static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float* v) { *p = v[0]; }
};

// The lane group of a batch row of D columns: G = 2^gshift lanes, the smallest power of two with G * V >= D up to a wave; lane l owns
// the V-wide chunks l, l + G, ... (per_lane of them at the most). Host side; an entry checks per_lane against the instantiations it has.
struct SbrLaneGroup { bool vec; int gshift, per_lane; };
static inline SbrLaneGroup sbr_lane_group(int D) {
  SbrLaneGroup g;
  g.vec = D % 4 == 0;
  const int chunks = g.vec ? D / 4 : D;
  g.gshift = 0;
  while (g.gshift < 6 && (1 << g.gshift) < chunks) ++g.gshift;
  g.per_lane = (chunks + (1 << g.gshift) - 1) >> g.gshift;
  return g;
}

#define SBR_SORTED_WAVES 4           // table rows per workgroup of a sorted-row scatter, one wave each
#define SBR_SORTED_D_MAX 256         // the widest row of a sorted-row scatter: 4 columns per lane

// sorted_keys [n_slots] ascending: the segment [beg, end) of the positions whose key is j, by two binary searches. A key that nobody
// looks for (the sentinel of a padded slot) belongs to no segment.
__device__ __forceinline__ void sbr_sorted_segment(const int* __restrict__ sorted_keys, long n_slots, int j, long& beg, long& end) {
  long lo = 0, hi = n_slots;
  while (lo < hi) {                                               // the first position whose key is >= j
    const long mid = (lo + hi) >> 1;
    if (sorted_keys[mid] < j) lo = mid + 1; else hi = mid;
  }
  beg = lo;
  hi = n_slots;
  while (lo < hi) {                                               // the first position whose key is > j
    const long mid = (lo + hi) >> 1;
    if (sorted_keys[mid] <= j) lo = mid + 1; else hi = mid;
  }
  end = lo;
}

// One wave walks the segment [beg, end) of a row: it reads the slot positions order[q] 64 at a time, one per lane, and takes them in
// ascending q. Lane l owns the columns l, l + 64, ... and adds acc = fmaf(coef[pos], src[pos / slots_per_row][col], acc); with SELF
// every lane also adds tsum = tsum + coef_s[pos], in the same order. A position outside [0, n_slots) is skipped. acc and tsum are the
// caller's, zeroed there.
template <bool SELF>
__device__ __forceinline__ void sbr_sorted_row_walk(const float* __restrict__ coef, const float* __restrict__ coef_s,
                                                    const float* __restrict__ src, const long* __restrict__ order, long beg, long end,
                                                    long n_slots, int slots_per_row, int D, int lane, float (&acc)[SBR_SORTED_D_MAX / 64],
                                                    float& tsum) {
#pragma clang fp contract(off)
  for (long q0 = beg; q0 < end; q0 += 64) {
    const int n_e = end - q0 < 64 ? (int)(end - q0) : 64;
    long my_row = -1;
    float my_c = 0.f, my_s = 0.f;
    if (lane < n_e) {
      const long pos = order[q0 + lane];
      if (pos >= 0 && pos < n_slots) {
        my_row = pos / slots_per_row;
        my_c = coef[pos];
        if (SELF) my_s = coef_s[pos];
      }
    }
    for (int e = 0; e < n_e; ++e) {
      const long row = __shfl(my_row, e, 64);
      const float c = __shfl(my_c, e, 64);
      const float cs = SELF ? __shfl(my_s, e, 64) : 0.f;
      if (row < 0) continue;
      if (SELF) tsum = tsum + cs;
      const float* sr = src + row * D;
#pragma unroll
      for (int k = 0; k < SBR_SORTED_D_MAX / 64; ++k) {
        const int col = lane + 64 * k;
        if (col < D) acc[k] = fmaf(c, sr[col], acc[k]);
      }
    }
  }
}
