// What the dense-block kernels of als.hip, svd.hip, rbmf.hip and ease.hip share, each stated once: the block width, the odd LDS row stride
// and staging a triangle at it, the layout "a wave owns a row, a lane two of its columns", partials per row slab added in slab order, the
// `info` word, the Cholesky factorisation in LDS, and the host checks of an entry's arguments with the shape of their refusal texts.
#pragma once
#include <initializer_list>
#include "common.h"

#define SBR_BLOCK_MAX 128             // columns of a block: ALS factors, the SVD's block, RBMF's representatives
// SBR_TRY: for helpers that return an error code; SBR_RAISE_LDS: sbr_raise_lds with the entry's own slot, `bytes` the size at SBR_BLOCK_MAX
#define SBR_TRY(call) do { if (const int rc__ = (call)) return rc__; } while (0)
#define SBR_RAISE_LDS(kernel, bytes) do { static SbrLdsSlot slot__; SBR_TRY(sbr_raise_lds(__func__, (const void*)kernel, &slot__, bytes)); } while (0)

// ---- LDS: the odd row stride ---------------------------------------------------------------------------------------------------------
// row stride of a matrix of `cols` columns in LDS: a walk down a column (stride ld) and 64 rows at the same column both touch every bank
// once. Cells, not bytes: the same for float and double matrices.
__host__ __device__ static inline int sbr_odd_ld(int cols) { return cols | 1; }
static inline size_t sbr_odd_cells(int rows, int cols) { return (size_t)rows * sbr_odd_ld(cols); }      // cells of [rows][cols] at that stride

// T [r][r] (global, rows ldt apart) -> lds [r][sbr_odd_ld(r)] by the workgroup's `threads` threads: the upper (`upper` != 0) or the lower
// triangle with the diagonal is read, the other one is staged as zeros. The caller places the barrier.
__device__ __forceinline__ void sbr_stage_triangle(float* lds, const float* __restrict__ T, long ldt, int r, int upper, int t, int threads) {
  const int ld = sbr_odd_ld(r);
  for (int e = t; e < r * r; e += threads) {
    const int i = e / r, j = e - i * r;
    lds[i * ld + j] = (upper ? j >= i : j <= i) ? T[(long)i * ldt + j] : 0.f;
  }
}

// ---- a wave owns a row of c <= 128 columns: lane l holds columns l and l + 64 ----------------------------------------------------------
struct SbrRow2 {
  int lane; bool h0, h1;              // h0, h1: this lane's first / second column exists (load gives zeros where not)
  __device__ __forceinline__ explicit SbrRow2(int c) : lane(threadIdx.x & 63), h0(lane < c), h1(lane + 64 < c) {}
  __device__ __forceinline__ void load(const float* row, float& v0, float& v1) const { v0 = h0 ? row[lane] : 0.f; v1 = h1 ? row[lane + 64] : 0.f; }
  __device__ __forceinline__ void store(float* row, float v0, float v1) const { if (h0) row[lane] = v0; if (h1) row[lane + 64] = v1; }
};

// ---- row slabs: one fp32 partial of `elems` elements per slab, added in slab order by a second launch -------------------------------------
static inline long sbr_slabs(long n, int slab) { return (n + slab - 1) / slab; }
static inline long sbr_slab_ws_bytes(long n, int slab, long elems) { return sbr_slabs(n, slab) * elems * 4; }
// element e = 256 blockIdx + threadIdx: finish(e, ws[0][e] + ws[1][e] + ... in slab order from +0); workgroups of 256 threads, or one of fewer
template <class FINISH>
__global__ __launch_bounds__(256) void sbr_slab_reduce_kernel(const float* __restrict__ ws, int n_slabs, int elems, FINISH finish) {
#pragma clang fp contract(off)
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= elems) return;
  float s = 0.f;
  for (int b = 0; b < n_slabs; ++b) s = s + ws[(long)b * elems + e];
  finish(e, s);
}

// ---- the info word: 0 on entry, 1 + the index of what failed --------------------------------------------------------------------------------
// first report wins: kernels with one reporter at a time (the launches of a stream, the columns of a factorisation)
__device__ __forceinline__ void sbr_report_first(int* info, int v) { atomicCAS(info, 0, v); }
// the smallest value wins, whatever the arrival order: many workgroups report their own index
__device__ __forceinline__ void sbr_report_min(int* info, int v) {
  int old = atomicCAS(info, 0, v);
  while (old != 0 && old > v) {
    const int seen = atomicCAS(info, old, v);
    if (seen == old) break;
    old = seen;
  }
}

// ---- the unpivoted Cholesky factorisation in LDS of sbr_als_solve_rows_f32 (als.hip) and sbr_chol_f32 (rbmf.hip) ------------------------------
// Cholesky by columns (Cholesky-Crout) of the lower triangle of A [rows][lda], rows >= f, in place; every thread of the workgroup calls
// it, thread t < rows owns row t. The rows from f on are right-hand sides carried along: row i >= f becomes L^-1 b_i. Column p: every
// owner of a row >= p walks row p (a broadcast read) and its own row, so it also has the pivot q = A[p][p] - sum_k L[p][k]^2 in the same
// bits as everybody else, and one barrier per column is enough. Below the diagonal A becomes L; the diagonal of L goes to diag[0 .. f)
// and A's own diagonal stays. A pivot that is <= 0 or not finite: bad(p) is called by the owner of row p, and the factorisation goes on
// with d = 1 (the output is then unspecified).
template <class BAD>
__device__ __forceinline__ void sbr_chol_lds(float* A, int lda, int f, int rows, float* diag, int t, BAD bad) {
#pragma clang fp contract(off)
  for (int p = 0; p < f; ++p) {
    if (t >= p && t < rows) {
      const float* rp = A + p * lda;
      float* ri = A + t * lda;
      float s = ri[p], q = rp[p];
      for (int k = 0; k < p; ++k) {
        const float lp = rp[k];
        s = fmaf(-ri[k], lp, s);
        q = fmaf(-lp, lp, q);
      }
      const bool ok = sbr_pos_finite(q);
      const float d = ok ? sqrtf(q) : 1.f;
      if (t == p) {
        diag[p] = d;
        if (!ok) bad(p);
      } else {
        ri[p] = s / d;
      }
    }
    __syncthreads();
  }
}

// ---- host checks of an entry's arguments -----------------------------------------------------------------------------------------------
// Every refusal reads "<entry>: <argument>=<value> ..." or "<entry>: <what> ...": `who` is the entry's name, `name` the argument's as the
// header spells it. An entry states them in the order block width, ranges, leading dimensions, (an empty range returns here), operands,
// workspace, so that a call with null pointers is refused for its shape first. Like SBR_REQUIRE, they return from the entry.
#define SBR_REQUIRE_WIDTH(who, name, v) SBR_REQUIRE((v) >= 1 && (v) <= SBR_BLOCK_MAX, "%s: %s=%d outside [1, %d]", who, name, v, SBR_BLOCK_MAX)
#define SBR_REQUIRE_ROWS(who, r0, r1, limit) /* rows [r0, r1) among `limit` rows */ \
  SBR_REQUIRE((r0) >= 0 && (r0) <= (r1) && (r1) <= (limit), "%s: row range [%ld, %ld) outside [0, %ld]", who, (long)(r0), (long)(r1), (long)(limit))
// (n rows cut into slabs, or tiles, of `slab` rows: their number fits an int)
#define SBR_REQUIRE_SLAB_ROWS(who, name, n, slab) SBR_REQUIRE((n) >= 0 && (n) <= 2147483647L * (slab), "%s: %s=%ld out of range", who, name, n)
#define SBR_REQUIRE_OPERANDS(who, cond) SBR_REQUIRE(cond, "%s: null operand", who)
// `need` bytes (the entry's _workspace query; 0: none, and the pointer is not looked at) at a multiple of `align` bytes
#define SBR_REQUIRE_WORKSPACE(who, ws, bytes, need, align)                                                         \
  SBR_REQUIRE((need) == 0 || ((ws) && (bytes) >= (need) && ((uintptr_t)(ws) & (uintptr_t)((align) - 1)) == 0), \
              "%s: workspace of %ld bytes, %ld needed at a multiple of %d", who, (long)(bytes), (long)(need), align)
// every leading dimension holds a row of `width` columns (`wname`: the width's argument); with SBR_TRY
struct SbrLd { const char* name; long ld; };
static inline int sbr_check_ld(const char* who, const char* wname, long width, std::initializer_list<SbrLd> lds) {
  for (const SbrLd& l : lds) SBR_REQUIRE(l.ld >= width, "%s: leading dimension %s=%ld below %s=%ld", who, l.name, l.ld, wname, width);
  return SBR_OK;
}
