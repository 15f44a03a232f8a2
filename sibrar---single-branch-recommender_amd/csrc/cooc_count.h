// Co-occurrence counts of one row of a binary CSR matrix M against every row of a tile, into u32 LDS counters: the counting step
// that sbr_knn_topk (knn.hip) and sbr_gram_dense (ease.hip) share.
#pragma once

// cnt[j - t0] += 1 for every entry (f, j) of M^T with f a feature of the owned row and t0 <= j < t0 + width. The owned row's features
// are indices[f_beg .. f_end); (t_indptr, t_indices) is M^T as CSR with ascending, unique indices. Wave w of `waves` takes the
// features w, w + waves, ... and walks M^T's row of each, entered at the tile's start by a lower bound. Integer LDS atomics only:
// exact and order-free. Called by whole workgroups, between two barriers (the counters zeroed before the first).
__device__ __forceinline__ void sbr_cooc_count_tile(const int* __restrict__ indices, long f_beg, long f_end,
                                                    const long* __restrict__ t_indptr, const int* __restrict__ t_indices, int t0,
                                                    int width, int w, int waves, int lane, unsigned int* cnt) {
  for (long p = f_beg + w; p < f_end; p += waves) {
    const int f = indices[p];
    long lo = t_indptr[f];
    const long end = t_indptr[f + 1];
    if (t0 > 0) {            // first entry with entity id >= t0
      long hi = end;
      while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (t_indices[mid] < t0) lo = mid + 1; else hi = mid;
      }
    }
    for (long q = lo + lane; q < end; q += 64) {
      const unsigned int x = (unsigned int)(t_indices[q] - t0);
      if (x >= (unsigned int)width) break;            // sorted: everything behind it lies in a later tile
      atomicAdd(&cnt[x], 1u);
    }
  }
}
