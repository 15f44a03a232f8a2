// Column reductions over an [n, D] row-major matrix in fp64 (column sums of bias gradients, BatchNorm statistics, the fused tail's
// column sums): the workspace layout, the block geometry, the publish tail, the finishing "take", the generic fallback and the host
// dispatch, each stated once for the kernels that reduce columns (DESIGN.md 4.5 names the four sites of the fused step that keep their
// own text of the geometry or of the tail, and what it cost to share it there).
#pragma once
#include "det.h"

// ---------------------------------------------------------------------------------------------------------------
// Workspace layout (doubles): [KD totals][SBR_COLRED_REP replicas][KD], KD = K * D for K reduced quantities per element. One double
// atomic per column and block goes to one of the replicas (blocks b, b + REP, ... share a replica: 512 blocks hitting the same D
// addresses serialise in the L2 atomic units — measured 50 us instead of 20 for a 90112 x 128 column sum). The replica part must be
// zero when a reduction starts and the finishing kernel (sbr_colred_take) leaves it zero again.
// `slots` (deterministic mode, det.h): [blocks][KD] doubles — every block stores its sums in the slot of its own index instead of
// adding them to a replica; nothing then depends on the order in which blocks finish (det.h: sbr_det_fold_slots adds the slots).
// ---------------------------------------------------------------------------------------------------------------
#define SBR_COLRED_REP 16

// base of the replica that block `block` adds to / of the slot it stores to (K quantities of D columns)
template <class I>
__device__ __forceinline__ double* sbr_colred_replica(double* ws, I block, int K, int D) { return ws + (long)(1 + (block % SBR_COLRED_REP)) * K * D; }
__device__ __forceinline__ double* sbr_colred_slot(double* slots, unsigned block, int K, int D) { return slots + (long)block * K * D; }

// sum of the replicas of entry i, leaving the replicas zeroed for the next call (the workspace contract: zero on first use,
// zero again on return — no memset node per call)
__device__ __forceinline__ double sbr_colred_take(double* __restrict__ ws, int KD, int i) {
  double s = 0.0;
#pragma unroll
  for (int r = 1; r <= SBR_COLRED_REP; ++r) {
    s += ws[(long)r * KD + i];
    ws[(long)r * KD + i] = 0.0;
  }
  return s;
}
// the same for the last-arriver block of a kernel whose other blocks added to the replicas (agent-scope atomics, performed at the
// memory side): it reads them with agent-scope atomic loads
__device__ __forceinline__ double sbr_colred_take_agent(double* ws, int KD, int i) {
  double s = 0.0;
#pragma unroll
  for (int r = 1; r <= SBR_COLRED_REP; ++r) {
    s += __hip_atomic_load(&ws[(long)r * KD + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ws[(long)r * KD + i] = 0.0;
  }
  return s;
}

static __global__ void sbr_colred_final_kernel(double* __restrict__ ws, int KD) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < KD) ws[i] = sbr_colred_take(ws, KD, i);
}

// (sum, sum of squares) of column c over n rows -> the BatchNorm's batch mean / rstd and running statistics (running_mean / running_var
// may be null together): shared by bn_finalize_kernel (batchnorm.hip) and the last-arriver block of gemm_split_kernel<0, 2>
__device__ __forceinline__ void sbr_bn_finish_column(double sum, double sq, long n, int c, float eps, float momentum, float* mean, float* rstd,
                                                     float* running_mean, float* running_var) {
  const double m = sum / (double)n;
  double var = sq / (double)n - m * m;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)m;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unbiased = n > 1 ? var * (double)n / (double)(n - 1) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Vector form (D % 4 == 0, D <= 1024). Block = 256 threads = RL row lanes x C4 = D / 4 column groups: thread t owns the float4 column
// group cg and walks rows lo + rl, lo + rl + RL, ... of the block's row range [lo, hi) (threads with rl >= RL idle when C4 does not
// divide 256).
// ---------------------------------------------------------------------------------------------------------------
struct SbrColGeom {
  int C4, RL, cg, rl;
  long lo, hi;
  __device__ __forceinline__ SbrColGeom(long n, int D) {
    C4 = D >> 2; RL = 256 / C4;
    const int t = threadIdx.x;
    cg = t % C4; rl = t / C4;
    const long chunk = (n + gridDim.x - 1) / gridDim.x;
    lo = blockIdx.x * chunk;
    hi = (lo + chunk < n) ? lo + chunk : n;
  }
};

// the row lanes' sums of one quantity in LDS -> this thread's four column sums (t < C4), in double, row lanes in ascending order.
// Lanes: float4[256] (fp32 thread sums, entry t of thread t) or double[4][256] (fp64 thread sums, [component][thread])
__device__ __forceinline__ void sbr_colred_fold(const float4 (&sm)[256], const SbrColGeom& g, double (&s)[4]) {
  const int t = threadIdx.x;
  s[0] = 0.0; s[1] = 0.0; s[2] = 0.0; s[3] = 0.0;
  for (int r = 0; r < g.RL; ++r) {
    const float4 p = sm[r * g.C4 + t];
    s[0] += (double)p.x; s[1] += (double)p.y; s[2] += (double)p.z; s[3] += (double)p.w;
  }
}
__device__ __forceinline__ void sbr_colred_fold(const double (&sm)[4][256], const SbrColGeom& g, double (&s)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double a = 0.0;
    for (int r = 0; r < g.RL; ++r) a += sm[i][r * g.C4 + t];
    s[i] = a;
  }
}

// Publish tail of a block: fold the row lanes of each of the K quantities, then store the sums to this block's slot (deterministic
// mode) or add them to its replica (four double atomics per thread and quantity). The CALLER's barrier publishes sm: the tail has none.
template <int K, class Lanes>
__device__ __forceinline__ void sbr_colred_publish(const Lanes (&sm)[K], const SbrColGeom& g, int D, double* __restrict__ ws,
                                                   double* __restrict__ slots) {
  const int t = threadIdx.x;
  if (t < g.C4) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s[4];
      sbr_colred_fold(sm[k], g, s);
      if (slots) {
        double* o = sbr_colred_slot(slots, blockIdx.x, K, D) + (long)k * D + 4 * t;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
        continue;
      }
      double* o = sbr_colred_replica(ws, blockIdx.x, K, D) + (long)k * D + 4 * t;
      atomicAdd(o, s[0]); atomicAdd(o + 1, s[1]); atomicAdd(o + 2, s[2]); atomicAdd(o + 3, s[3]);
    }
  }
}

// A thread walks the block's row range with four independent 16-byte loads in flight, accumulating in fp32 (at most a few dozen rows
// per thread); the publish tail combines the row lanes in double.
//   f(row, cg, v) fills v[K] (float4 each) for columns 4*cg .. 4*cg+3 of `row`.
__device__ __forceinline__ void sbr_f4_add(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

template <int K, class F>
__device__ __forceinline__ void sbr_col_reduce(long n, int D, double* __restrict__ ws, F f, double* __restrict__ slots = nullptr) {
  __shared__ float4 sm[K][256];
  const SbrColGeom g(n, D);
  const int RL = g.RL, cg = g.cg;
  float4 acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (g.rl < RL) {
    long j = g.lo + g.rl;
    for (; j + 3L * RL < g.hi; j += 4L * RL) {
      float4 v0[K], v1[K], v2[K], v3[K];
      f(j, cg, v0); f(j + RL, cg, v1); f(j + 2L * RL, cg, v2); f(j + 3L * RL, cg, v3);
#pragma unroll
      for (int k = 0; k < K; ++k) { sbr_f4_add(v0[k], v1[k]); sbr_f4_add(v2[k], v3[k]); sbr_f4_add(v0[k], v2[k]); sbr_f4_add(acc[k], v0[k]); }
    }
    for (; j < g.hi; j += RL) {
      float4 v[K];
      f(j, cg, v);
#pragma unroll
      for (int k = 0; k < K; ++k) sbr_f4_add(acc[k], v[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) sm[k][threadIdx.x] = acc[k];
  __syncthreads();
  sbr_colred_publish(sm, g, D, ws, slots);
}

// launch geometry of the vector form: every block gets >= 8 passes of its row lanes
static inline int sbr_col_reduce_blocks(long n, int D) {
  const int RL = 256 / (D >> 2);
  long b = (n + 8L * RL - 1) / (8L * RL);
  const long cap = 512;
  if (b > cap) b = cap;          // one double atomic per block and column: more blocks only add contention on D addresses
  return b < 1 ? 1 : (int)b;
}
static inline bool sbr_col_reduce_ok(const void* p, long ld, int D) {
  return (D & 3) == 0 && D >= 4 && D <= 1024 && (ld & 3) == 0 && (((uintptr_t)p) & 15) == 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Generic fallback (any D, any alignment). grid: (row chunks, column groups of 64); block 256 = 4 row groups x 64 columns. Double sums
// per thread, the four row groups added in order, one double atomic per column, quantity and block straight into replica 1 (`rep1`).
//   f(row, col, v) fills v[K] (doubles) for element (row, col).
// ---------------------------------------------------------------------------------------------------------------
template <int K, class F>
__device__ __forceinline__ void sbr_col_reduce_generic(long n, int D, double* __restrict__ rep1, F f) {
  __shared__ double sm[K][256];
  const int t = threadIdx.x, c = blockIdx.y * 64 + (t & 63), rg = t >> 6;
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  if (c < D)
    for (long j = blockIdx.x * 4L + rg; j < n; j += gridDim.x * 4L) {
      double v[K];
      f(j, c, v);
#pragma unroll
      for (int k = 0; k < K; ++k) s[k] += v[k];
    }
#pragma unroll
  for (int k = 0; k < K; ++k) sm[k][t] = s[k];
  __syncthreads();
  if (rg == 0 && c < D) {
#pragma unroll
    for (int k = 0; k < K; ++k) atomicAdd(&rep1[(long)k * D + c], sm[k][t] + sm[k][t + 64] + sm[k][t + 128] + sm[k][t + 192]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Host dispatch of an entry point `who` that reduces K quantities over n >= 1 rows of D columns (`dim`: the letter the entry's messages
// call D by) into the pending replicas of ws; the caller's finishing kernel runs behind it.
//   deterministic mode: the vector form is required; one slot per block from the library's scratch, vec(blocks, slots), then the slots
//                       are folded into replica 1 in slot order
//   vec_ok:             vec(blocks, nullptr) — arrival-order atomics into the replicas
//   otherwise:          gen(grid, ws + KD)   — the generic kernel, arrival-order atomics into replica 1
// ---------------------------------------------------------------------------------------------------------------
template <class Vec, class Gen>
static inline int sbr_colred_dispatch(const char* who, char dim, long n, int D, int K, bool vec_ok, double* ws, hipStream_t s, Vec vec,
                                      Gen gen) {
  const int KD = K * D;
  if (sbr_det_on()) {
    SBR_REQUIRE(vec_ok, "%s: no deterministic form for %c=%d (needs %c %% 4 == 0, %c <= 1024, 16-byte aligned operands)", who, dim, D, dim, dim);
    const int nb = sbr_col_reduce_blocks(n, D);
    double* slots = (double*)sbr_det_scratch(SBR_SCRATCH_COLRED, (size_t)nb * KD * sizeof(double), s, who);
    if (!slots) return SBR_ERR_HIP;
    vec(nb, slots);
    return sbr_det_fold_slots(slots, nb, KD, ws, s, who);
  }
  sbr_note_arrival_order();
  if (vec_ok) {
    vec(sbr_col_reduce_blocks(n, D), (double*)nullptr);
  } else {
    int bx = sbr_cdiv(n, 64);
    if (bx > 512) bx = 512;
    gen(dim3(bx, sbr_cdiv(D, 64)), ws + KD);
  }
  return SBR_OK;
}
