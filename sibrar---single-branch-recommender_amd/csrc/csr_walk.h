// Walking sorted CSR rows inside a window of columns: what the fit-matrix kernels share. sbr_knn_topk (knn.hip) and sbr_gram_dense
// (ease.hip) count co-occurrences with it; sbr_p3_walk_dense (p3alpha.hip) and sbr_csr_rows_times_csr (knn.hip) enter their rows with it.
// A row is a range [lo, end) of positions into an index array with ascending, unique columns.
#pragma once

// The first position in [lo, hi) whose column is >= c0 (hi when there is none). I: the callers' position type (long, or int offsets).
template <class I>
__device__ __forceinline__ I sbr_csr_lower_bound(const int* __restrict__ idx, I lo, I hi, int c0) {
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (idx[mid] < c0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// f(x = column - c0, q) for the entries q of [lo, end) whose column lies in [c0, c0 + width): the lanes of a wave take lo + lane,
// lo + lane + 64, ... and each stops at its first column outside the window (sorted: everything behind it lies in a later window). No
// column of [lo, end) may lie in front of the window: lo is the row's lower bound of c0, or c0 is 0.
template <class F>
__device__ __forceinline__ void sbr_csr_walk_window(const int* __restrict__ idx, long lo, long end, int c0, int width, int lane, F f) {
  for (long q = lo + lane; q < end; q += 64) {
    const unsigned int x = (unsigned int)(idx[q] - c0);
    if (x >= (unsigned int)width) break;
    f(x, q);
  }
}

// cnt[j - t0] += 1 for every entry (f, j) of M^T with f a feature of the owned row and t0 <= j < t0 + width. The owned row's features
// are indices[f_beg .. f_end); (t_indptr, t_indices) is M^T as CSR. Wave w of `waves` takes the features w, w + waves, ... and walks
// M^T's row of each, entered at the tile's start. Integer LDS atomics only: exact and order-free. Called by whole workgroups, between
// two barriers (the counters zeroed before the first).
__device__ __forceinline__ void sbr_cooc_count_tile(const int* __restrict__ indices, long f_beg, long f_end,
                                                    const long* __restrict__ t_indptr, const int* __restrict__ t_indices, int t0,
                                                    int width, int w, int waves, int lane, unsigned int* cnt) {
  for (long p = f_beg + w; p < f_end; p += waves) {
    const int f = indices[p];
    const long lo = t_indptr[f], end = t_indptr[f + 1];
    sbr_csr_walk_window(t_indices, t0 > 0 ? sbr_csr_lower_bound(t_indices, lo, end, t0) : lo, end, t0, width, lane,
                        [&](unsigned int x, long) { atomicAdd(&cnt[x], 1u); });
  }
}
