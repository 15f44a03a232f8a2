// The unpivoted Cholesky factorisation in LDS that sbr_als_solve_rows_f32 (als.hip) and sbr_chol_f32 (rbmf.hip) share.
#pragma once
#include "common.h"

// odd row stride of a matrix of f columns in LDS: a walk down a column (stride lda) and 64 rows at the same column both touch every
// bank once
__host__ __device__ static inline int sbr_chol_lda(int f) { return f | 1; }

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
