// Top-k selection of one row of a co-occurrence-derived value matrix inside one workgroup: what sbr_knn_topk (knn.hip) and
// sbr_cooc_weight_topk (ultragcn.hip) share behind the counting of csr_walk.h. A workgroup of THREADS threads owns a row. Its entity
// columns pass through tiles of u32 cells in LDS: the caller counts into a tile (sbr_cooc_count_tile), replaces every cell in place by
// the bits of its value (> 0, so the bits order like the values; 0 = no candidate), and then
//   sbr_topk_select_tile   merges the tile into the carried list of the k largest composites (value bits << 32 | 0xFFFFFFFF - j: value
//                          descending, index ascending) by radix select on the composite (4 passes on the value; 4 more on the index
//                          only when equal values straddle the k-th place) and compaction into the second list buffer;
//   sbr_topk_sort_write    after the last tile: bitonic sort of the list, then the row's (idx, val, len) with the (-1, 0) padding.
// Integer LDS atomics only: exact and order-free, and the final sort fixes the order, so the result has the same bits on every run.
#pragma once

// the selection's LDS of a kernel whose lists hold up to K_MAX entries (a power of two): one `__shared__ SbrTopkLds<K_MAX>` per kernel
template <int K_MAX>
struct SbrTopkLds {
  unsigned long long lists[2][K_MAX];
  unsigned int hist[256];
  unsigned int prefix_hi, prefix_lo, need, take_all, done, cnt;
};

// One histogram add. Similarities crowd into a few exponents, so in the leading radix passes most lanes of a wave name the same
// bin: when they all do, one lane adds the wave's count instead of up to 64 adds queueing on one address. Called by whole waves.
__device__ __forceinline__ void knn_hist_add(unsigned int* hist, bool active, unsigned int digit) {
  const unsigned long long act = __ballot(active);
  if (act == 0ull) return;
  const int src = __ffsll((long long)act) - 1;
  const unsigned int first = (unsigned int)__shfl((int)digit, src, 64);
  if (__ballot(active && digit == first) == act) {
    if ((int)(threadIdx.x & 63) == src) atomicAdd(&hist[first], (unsigned int)__popcll(act));
  } else if (active) {
    atomicAdd(&hist[digit], 1u);
  }
}

// The radix step of wave 0: the bin d (from 255 down) at which the running count reaches `need`; -> true in the lane that holds it,
// with the count of the bins above it and the bin's own count. Lane l owns the bins 255 - 4 l ... 252 - 4 l. total: all bins.
__device__ __forceinline__ bool knn_find_bin(const unsigned int* hist, unsigned int need, int lane, int& d, unsigned int& above,
                                             unsigned int& own, unsigned int& total) {
  unsigned int h[4], s = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) { h[q] = hist[255 - 4 * lane - q]; s += h[q]; }
  unsigned int incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned int up = (unsigned int)__shfl_up((int)incl, o, 64);
    if (lane >= o) incl += up;
  }
  total = (unsigned int)__shfl((int)incl, 63, 64);
  unsigned int a = incl - s;
  bool found = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (!found && a + h[q] >= need) { found = true; d = 255 - 4 * lane - q; above = a; own = h[q]; }
    a += h[q];
  }
  const unsigned long long f = __ballot(found);
  return found && lane == __ffsll((long long)f) - 1;
}

// The tile cnt[0 .. width) of columns t0 .. holds value bits (0: no candidate). S.lists[cur][0 .. n_list) is the list carried from the
// earlier tiles, unsorted. -> the k largest composites of both in S.lists[cur ^ 1], cur and n_list updated. Called by the whole
// workgroup; the tile's cells must have been written by the caller without a barrier in between (the first barrier is in here).
template <int THREADS, int K_MAX>
__device__ __forceinline__ void sbr_topk_select_tile(SbrTopkLds<K_MAX>& S, const unsigned int* cnt, int width, int t0, int k, int& cur,
                                                     unsigned int& n_list) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) { S.take_all = 0u; S.done = 0u; }
  __syncthreads();
  // ---- select: the composite of the k-th largest entry of (carried list, tile)
  unsigned int pre_hi = 0u, pre_lo = 0u, need = (unsigned int)k;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 24 - 8 * (pass & 3);
    const bool on_index = pass >= 4;
    const unsigned int hi_mask = (pass & 3) == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    if (t < 256) S.hist[t] = 0u;
    __syncthreads();
    for (int x = t; x < (int)n_list; x += THREADS) {
      const unsigned long long e = S.lists[cur][x];
      const unsigned int vb = (unsigned int)(e >> 32), ib = (unsigned int)e;
      const bool in = on_index ? (vb == pre_hi && (ib & hi_mask) == pre_lo) : ((vb & hi_mask) == pre_hi);
      if (in) atomicAdd(&S.hist[((on_index ? ib : vb) >> shift) & 255u], 1u);
    }
    for (int x0 = 0; x0 < width; x0 += THREADS) {
      const int x = x0 + t;
      const unsigned int vb = x < width ? cnt[x] : 0u, ib = 0xFFFFFFFFu - (unsigned int)(t0 + x);
      const bool in = vb != 0u && (on_index ? (vb == pre_hi && (ib & hi_mask) == pre_lo) : ((vb & hi_mask) == pre_hi));
      knn_hist_add(S.hist, in, ((on_index ? ib : vb) >> shift) & 255u);
    }
    __syncthreads();
    if (w == 0) {
      int d = 0;
      unsigned int above = 0u, own = 0u, total = 0u;
      const bool mine = knn_find_bin(S.hist, need, lane, d, above, own, total);
      if (pass == 0 && total <= (unsigned int)k) {
        if (lane == 0) S.take_all = 1u;                           // everything fits: no threshold
      } else if (mine) {                                          // (a bin is always found: the prefix group holds >= need entries)
        if (on_index) S.prefix_lo = pre_lo | ((unsigned int)d << shift);
        else { S.prefix_hi = pre_hi | ((unsigned int)d << shift); S.prefix_lo = 0u; }
        S.need = need - above;
        // the value is fixed after pass 3: if every entry that has it is needed, the index does not matter
        if (pass == 3 && own == need - above) S.done = 1u;
      }
    }
    __syncthreads();
    pre_hi = S.prefix_hi;
    pre_lo = S.prefix_lo;
    need = S.need;
    if (S.take_all || S.done) break;             // uniform: read behind the barrier, written before it
  }
  const unsigned long long thr = S.take_all ? 1ull : (((unsigned long long)pre_hi << 32) | (unsigned long long)pre_lo);
  // ---- compaction of every composite >= thr into the other buffer (the order is fixed by the final sort)
  if (t == 0) S.cnt = 0u;
  __syncthreads();
  const int nxt = cur ^ 1;
  for (int x = t; x < (int)n_list; x += THREADS) {
    const unsigned long long e = S.lists[cur][x];
    if (e >= thr) {
      const unsigned int pos = atomicAdd(&S.cnt, 1u);
      if (pos < (unsigned int)k) S.lists[nxt][pos] = e;
    }
  }
  for (int x = t; x < width; x += THREADS) {
    const unsigned int vb = cnt[x];
    if (vb != 0u) {
      const unsigned long long e = ((unsigned long long)vb << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)(t0 + x));
      if (e >= thr) {
        const unsigned int pos = atomicAdd(&S.cnt, 1u);
        if (pos < (unsigned int)k) S.lists[nxt][pos] = e;             // (pos < k always: the guard keeps a wrong count inside the buffer)
      }
    }
  }
  __syncthreads();
  n_list = S.cnt < (unsigned int)k ? S.cnt : (unsigned int)k;
  cur = nxt;
  __syncthreads();
}

// Sort of S.lists[cur][0 .. n_list) (descending composites; the zero padding up to kpad, a power of two >= max(k, 2), sorts last) and
// the write of row i: nbr_idx / nbr_val [.., k] and nbr_len. Called by the whole workgroup.
template <int THREADS, int K_MAX>
__device__ __forceinline__ void sbr_topk_sort_write(SbrTopkLds<K_MAX>& S, int cur, unsigned int n_list, int k, int kpad, int i,
                                                    int* __restrict__ nbr_idx, float* __restrict__ nbr_val, int* __restrict__ nbr_len) {
  const int t = threadIdx.x;
  for (int x = (int)n_list + t; x < kpad; x += THREADS) S.lists[cur][x] = 0ull;
  __syncthreads();
  for (int size = 2; size <= kpad; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (t < kpad) {
        const int j = t ^ stride;
        if (j > t) {
          const bool desc = (t & size) == 0;
          const unsigned long long a = S.lists[cur][t], b = S.lists[cur][j];
          if ((a < b) == desc) { S.lists[cur][t] = b; S.lists[cur][j] = a; }
        }
      }
      __syncthreads();
    }
  }
  if (t < k) {
    const unsigned long long e = S.lists[cur][t];
    const bool real = t < (int)n_list;
    nbr_idx[(long)i * k + t] = real ? (int)(0xFFFFFFFFu - (unsigned int)(e & 0xFFFFFFFFull)) : -1;
    nbr_val[(long)i * k + t] = real ? __uint_as_float((unsigned int)(e >> 32)) : 0.f;
  }
  if (t == 0) nbr_len[i] = (int)n_list;
}
