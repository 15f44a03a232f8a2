// LightGCN's propagation (He et al., SIGIR 2020): y = A^ x over the joint row space of the bipartite user-item graph, with
// A^ = D^-1/2 A D^-1/2 the symmetrically normalised adjacency of 0/1 interaction data. Joint row r < n_users is user r, its neighbours
// are the joint rows n_users + i of the items i of the user's CSR row; joint row r >= n_users is item r - n_users, its neighbours are
// the users of the transposed matrix's row. One entry:
//   sbr_graph_propagate_f32  y[r][d] = s_r * (fmaf chain of s_c * x[c][d] over the neighbours c, ascending), sum[r][d] = (sum[r][d] + y[r][d]) * scale
// A^ is symmetric, so the same launch is the backward pass. No atomics and no reduction across lanes: every output element has one
// owner (one lane) that takes its terms in ascending CSR order, so the bits do not depend on the run, on the split of the rows or on
// the lane mapping below. include/sibrar_hip.h states the same order; tests/lightgcn_ref.py restates it in numpy. csr_walk.h is not
// used: its walkers enter a sorted row inside a window of columns, and a propagation takes whole rows.
#include "common.h"

#define GP_THREADS 256
#define GP_WAVES (GP_THREADS / 64)
#define GP_UNROLL 8                  // neighbour rows in flight per lane group (the additions stay in CSR order)
#define GP_D_MAX 512
#define GP_DIM_MAX (1 << 24)         // a degree is at most a dimension of the matrix: converted to fp32 exactly

// s of the header: one correctly rounded square root and one correctly rounded division of an exactly converted degree (no rsqrt)
__device__ __forceinline__ float gp_scale(long d) { return d > 0 ? 1.0f / sqrtf((float)d) : 0.f; }

template <int V> struct GpVec;
template <> struct GpVec<4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct GpVec<1> {
  static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float* v) { *p = v[0]; }
};

// A row of 4 D bytes is a gather of latency, not of arithmetic: a full wave on a 64-float row would leave three quarters of its lanes
// without a float4 to load. So a row belongs to a group of G = 2^gshift lanes (G * C * V >= D: lane l of the group owns the V-wide
// chunks l, l + G, ... of the row, C of them), and a wave takes 64 / G consecutive rows. The group reads its neighbours G at a time,
// one per lane (the column, and the scale from the degree in the other side's indptr), and then hands them round by shuffles inside
// the group: GP_UNROLL neighbour rows are loaded before the first of them is added, and the additions follow in CSR order. The groups
// of a wave diverge only in their trip counts; a shuffle's source lane is always in the reader's own group.
template <int V, int C>
__global__ __launch_bounds__(GP_THREADS) void graph_prop_kernel(const long* __restrict__ u_indptr, const int* __restrict__ u_indices,
                                                                const long* __restrict__ i_indptr, const int* __restrict__ i_indices,
                                                                int n_users, long r0, long r1, const float* __restrict__ x,
                                                                float* __restrict__ y, float* __restrict__ sum, float sum_scale, int D,
                                                                int gshift) {
#pragma clang fp contract(off)
  const int G = 1 << gshift;
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane - gl;
  const long wave = (long)blockIdx.x * GP_WAVES + (threadIdx.x >> 6);
  const long r = r0 + (wave << (6 - gshift)) + (lane >> gshift);
  if (r >= r1) return;
  const bool user = r < n_users;
  const long* indptr = user ? u_indptr : i_indptr;                // the row's own side
  const int* indices = user ? u_indices : i_indices;
  const long* o_indptr = user ? i_indptr : u_indptr;              // the neighbours' side: their degrees
  const long local = user ? r : r - n_users;
  const long c_base = user ? n_users : 0;                         // joint row of neighbour c: c_base + c
  const long beg = indptr[local], end = indptr[local + 1];
  float acc[C][V];
#pragma unroll
  for (int k = 0; k < C; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[k][j] = 0.f;
  for (long p0 = beg; p0 < end; p0 += G) {
    const int n_e = end - p0 < G ? (int)(end - p0) : G;
    int my_c = 0;
    float my_s = 0.f;
    if (gl < n_e) {
      my_c = indices[p0 + gl];
      my_s = gp_scale(o_indptr[my_c + 1] - o_indptr[my_c]);
    }
    for (int e0 = 0; e0 < n_e; e0 += GP_UNROLL) {
      float v[GP_UNROLL][C][V], s[GP_UNROLL];
#pragma unroll
      for (int u = 0; u < GP_UNROLL; ++u) {
        if (e0 + u < n_e) {
          const float* xr = x + (c_base + (long)__shfl(my_c, gbase + e0 + u, 64)) * D;
          s[u] = __shfl(my_s, gbase + e0 + u, 64);
#pragma unroll
          for (int k = 0; k < C; ++k) {
            const int col = (gl + k * G) * V;
            if (col < D) GpVec<V>::load(xr + col, v[u][k]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < GP_UNROLL; ++u) {
        if (e0 + u < n_e) {
#pragma unroll
          for (int k = 0; k < C; ++k)
            if ((gl + k * G) * V < D) {
#pragma unroll
              for (int j = 0; j < V; ++j) acc[k][j] = fmaf(s[u], v[u][k][j], acc[k][j]);
            }
        }
      }
    }
  }
  const float s_r = gp_scale(end - beg);
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int col = (gl + k * G) * V;
    if (col >= D) continue;
    float out[V];
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = s_r * acc[k][j];
    GpVec<V>::store(y + r * D + col, out);
    if (sum) {
      float t[V];
      GpVec<V>::load(sum + r * D + col, t);
#pragma unroll
      for (int j = 0; j < V; ++j) t[j] = (t[j] + out[j]) * sum_scale;
      GpVec<V>::store(sum + r * D + col, t);
    }
  }
}

// the byte ranges [a, a + bytes) and [b, b + bytes) meet
static inline bool gp_overlap(const void* a, const void* b, long bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < (uintptr_t)bytes : pa - pb < (uintptr_t)bytes;
}

template <int V, int C>
static void gp_launch(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users, long r0, long r1,
                      const float* x, float* y, float* sum, float sum_scale, int D, int gshift, hipStream_t stream) {
  const long rows_per_block = (long)GP_WAVES << (6 - gshift);
  graph_prop_kernel<V, C><<<(unsigned)((r1 - r0 + rows_per_block - 1) / rows_per_block), GP_THREADS, 0, stream>>>(
      u_indptr, u_indices, i_indptr, i_indices, n_users, r0, r1, x, y, sum, sum_scale, D, gshift);
}

extern "C" int sbr_graph_propagate_f32(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users,
                                       int n_items, long r0, long r1, const float* x, float* y, float* sum, float sum_scale, int D,
                                       void* stream) {
  SBR_REQUIRE(D >= 1 && D <= GP_D_MAX, "sbr_graph_propagate_f32: D=%d outside [1, %d]", D, GP_D_MAX);
  SBR_REQUIRE(n_users >= 0 && n_users <= GP_DIM_MAX && n_items >= 0 && n_items <= GP_DIM_MAX, "sbr_graph_propagate_f32: shape [%d, %d] "
              "outside [0, 2^24] x [0, 2^24]: a degree over 2^24 has no exact fp32 form", n_users, n_items);
  const long n = (long)n_users + n_items;
  SBR_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= n, "sbr_graph_propagate_f32: row range [%ld, %ld) outside [0, %ld]", r0, r1, n);
  const long bytes = 4 * n * D;
  SBR_REQUIRE(!(x && y && gp_overlap(x, y, bytes)), "sbr_graph_propagate_f32: x aliases y: a row reads other rows, so the input table "
              "cannot be an output");
  SBR_REQUIRE(!(x && sum && gp_overlap(x, sum, bytes)), "sbr_graph_propagate_f32: x aliases sum: a row reads other rows, so the input table "
              "cannot be an output");
  SBR_REQUIRE(!(y && sum && gp_overlap(y, sum, bytes)), "sbr_graph_propagate_f32: y aliases sum: both are written");
  if (r0 == r1) return SBR_OK;
  SBR_REQUIRE(u_indptr && i_indptr && x && y, "sbr_graph_propagate_f32: null operand");              // (a matrix without entries has no indices)
  // float4 chunks where every row of every table starts on a 16-byte boundary, single floats otherwise; the group is the smallest
  // power of two of lanes that covers the row, a wave at the most, and a lane then owns C chunks
  const bool vec = D % 4 == 0 && ((uintptr_t)x | (uintptr_t)y | (uintptr_t)sum) % 16 == 0;
  const int chunks = vec ? D / 4 : D;
  int gshift = 0;
  while (gshift < 6 && (1 << gshift) < chunks) ++gshift;
  const int per_lane = (chunks + (1 << gshift) - 1) >> gshift;
  hipStream_t st = (hipStream_t)stream;
#define GP_GO(V, C) gp_launch<V, C>(u_indptr, u_indices, i_indptr, i_indices, n_users, r0, r1, x, y, sum, sum_scale, D, gshift, st)
  if (vec) {
    if (per_lane <= 1) GP_GO(4, 1); else GP_GO(4, 2);
  } else {
    if (per_lane <= 1) GP_GO(1, 1); else if (per_lane <= 2) GP_GO(1, 2); else if (per_lane <= 4) GP_GO(1, 4); else GP_GO(1, 8);
  }
#undef GP_GO
  SBR_CHECK_LAUNCH("sbr_graph_propagate_f32");
  return SBR_OK;
}
