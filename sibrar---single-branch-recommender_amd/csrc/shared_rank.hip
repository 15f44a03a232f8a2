// The two baselines of algorithms/naive_algs.py:11-60, whose score rows need no matrix:
//   sbr_shared_rank_topk   PopularItems: every user has the same score row, so a user's list is the shared ranking minus the user's
//                          exclusions: about k + |excl(u)| reads per user instead of a [users, items] score matrix
//   sbr_uniform_rows_f32   RandomItems: U(seed, user id, item position) by a counter-based generator, a pure function of the three
// No LDS, no atomics, one writer per output element: the same bits on every run, valid in deterministic mode.
#include "common.h"
#include "philox.h"

// One wave per user walks `order` 64 ranks at a time. Lane l of a step holds rank r + l and keeps it when the item is not in the user's
// exclusion row (a binary search in the CSR row); the ballot of the kept lanes numbers them in rank order, so the first k kept items
// land in slots 0 .. k-1 whatever the step they were found in.
__global__ __launch_bounds__(256) void shared_rank_topk_kernel(const int* __restrict__ order, const float* __restrict__ score, int n_items,
                                                               const long* __restrict__ u_idx, const long* __restrict__ indptr,
                                                               const int* __restrict__ indices, long Bu, int k,
                                                               float* __restrict__ out_val, int* __restrict__ out_idx) {
  const long b = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= Bu) return;                                          // uniform per wave
  const int lane = threadIdx.x & 63;
  const long u = u_idx ? u_idx[b] : b;
  const long beg = indptr[u], end = indptr[u + 1];
  float* __restrict__ ov = out_val + b * (long)k;
  int* __restrict__ oi = out_idx + b * (long)k;
  long found = 0;
  for (long r = 0; r < n_items && found < k; r += 64) {
    bool keep = r + lane < n_items;
    int p = 0;
    if (keep) {
      p = order[r + lane];
      keep = (unsigned int)p < (unsigned int)n_items;           // `order` is a permutation; an entry that is not a position is passed over, never read through
      if (keep && end > beg) {                                  // an empty row excludes nothing
        long lo = beg, hi = end;
        while (lo < hi) {
          const long mid = (lo + hi) >> 1;
          if (indices[mid] < p) lo = mid + 1; else hi = mid;
        }
        keep = !(lo < end && indices[lo] == p);
      }
    }
    const unsigned long long kept = __ballot(keep);
    const long slot = found + __popcll(kept & ((1ull << lane) - 1ull));
    if (keep && slot < k) {
      ov[slot] = score[p];                                      // a kept item whose score is -inf keeps its index
      oi[slot] = p;
    }
    found += __popcll(kept);
  }
  for (long j = (found < k ? found : k) + lane; j < k; j += 64) {      // behind the user's last scoreable item: the empty-slot convention
    ov[j] = -INFINITY;
    oi[j] = -1;
  }
}

extern "C" int sbr_shared_rank_topk(const int* order, const float* score, int n_items, const long* u_idx, const long* excl_indptr,
                                    const int* excl_indices, long Bu, int k, float* out_val, int* out_idx, void* stream) {
  SBR_REQUIRE(k >= 1, "sbr_shared_rank_topk: k=%d must be at least 1", k);
  SBR_REQUIRE(n_items >= 0 && Bu >= 0, "sbr_shared_rank_topk: negative size (n_items=%d, Bu=%ld)", n_items, Bu);
  if (Bu == 0) return SBR_OK;
  SBR_REQUIRE(excl_indptr && out_val && out_idx && (n_items == 0 || (order && score)), "sbr_shared_rank_topk: null operand");
  SBR_REQUIRE(Bu <= 4L * 0x7FFFFFFF, "sbr_shared_rank_topk: Bu=%ld users are more than one launch takes", Bu);
  shared_rank_topk_kernel<<<sbr_cdiv(Bu, 4), 256, 0, (hipStream_t)stream>>>(order, score, n_items, u_idx, excl_indptr, excl_indices, Bu, k,
                                                                           out_val, out_idx);
  SBR_CHECK_LAUNCH("sbr_shared_rank_topk");
  return SBR_OK;
}

// The generator (Philox4x32-10 and the [0, 1) mapping) is philox.h's.
#define UNIFORM_MAX_GRID 65536L         // workgroups of a launch: 2^24 threads keep every CU busy, a larger output is walked in grid strides

// One thread per (row, block of four columns): the block's counter is (user id low, user id high, j / 4, 0), so an element's value
// depends on (seed, user id, j) alone, not on the grid, the chunk or the row's place in the batch.
__global__ __launch_bounds__(256) void uniform_rows_kernel(unsigned int k0, unsigned int k1, const long* __restrict__ u_idx, long Bu,
                                                           int n_items, int n_blocks, float* __restrict__ out, long ld, bool vec) {
  const long total = Bu * (long)n_blocks;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long b = t / n_blocks;
    const int q = (int)(t - b * n_blocks);
    const unsigned long long u = (unsigned long long)(u_idx ? u_idx[b] : b);
    const uint4 x = philox4x32_10(make_uint4((unsigned int)u, (unsigned int)(u >> 32), (unsigned int)q, 0u), k0, k1);
    float* __restrict__ row = out + b * ld;
    const int j = 4 * q;                                        // j <= n_items - 1: no overflow
    if (vec && n_items - j >= 4) {
      *reinterpret_cast<float4*>(row + j) = make_float4(philox_unit(x.x), philox_unit(x.y), philox_unit(x.z), philox_unit(x.w));
    } else {
      const unsigned int w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < n_items - j) row[j + c] = philox_unit(w[c]);
    }
  }
}

extern "C" int sbr_uniform_rows_f32(unsigned long seed, const long* u_idx, long Bu, int n_items, float* out, long ld, void* stream) {
  SBR_REQUIRE(n_items >= 0 && Bu >= 0, "sbr_uniform_rows_f32: negative size (n_items=%d, Bu=%ld)", n_items, Bu);
  if (Bu == 0 || n_items == 0) return SBR_OK;
  SBR_REQUIRE(out, "sbr_uniform_rows_f32: null operand");
  SBR_REQUIRE(ld >= n_items, "sbr_uniform_rows_f32: leading dimension %ld below the %d items of a row", ld, n_items);
  const int n_blocks = (int)(((long)n_items + 3) / 4);
  const long total = Bu * (long)n_blocks;
  const bool vec = (ld % 4 == 0) && ((((uintptr_t)out) & 15) == 0);                 // every row 16-byte aligned: one store per block of four
  const long want = (total + 255) / 256;
  const int grid = (int)(want < UNIFORM_MAX_GRID ? want : UNIFORM_MAX_GRID);        // beyond 2^24 threads each takes several blocks of four
  uniform_rows_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((unsigned int)seed, (unsigned int)((unsigned long long)seed >> 32), u_idx, Bu,
                                                            n_items, n_blocks, out, ld, vec);
  SBR_CHECK_LAUNCH("sbr_uniform_rows_f32");
  return SBR_OK;
}
