// LightGCN's propagation (He et al., SIGIR 2020): y = A^ x over the joint row space of the bipartite user-item graph, with
// A^ = D^-1/2 A D^-1/2 the symmetrically normalised adjacency of 0/1 interaction data. Joint row r < n_users is user r, its neighbours
// are the joint rows n_users + i of the items i of the user's CSR row; joint row r >= n_users is item r - n_users, its neighbours are
// the users of the transposed matrix's row. Two entries on one kernel:
//   sbr_graph_propagate_f32        y[r][d] = s_r * (fmaf chain of s_c * x[c][d] over the neighbours c, ascending), sum[r][d] = (sum[r][d] + y[r][d]) * scale
//   sbr_graph_propagate_noise_f32  the same y, perturbed before it is stored and summed (SimGCL / XSimGCL: Yu et al., SIGIR 2022, TKDE 2023):
//                                  y += sgn(y) * eps * u / |u_r|, u = U(seed, stream_id, r, d) from Philox4x32-10, made in the registers
//                                  of the lane that owns the element; the row norm is one butterfly inside the row's lane group
// A^ is symmetric, so the same launch is the backward pass. No atomics and no reduction across lanes: every output element has one
// owner (one lane) that takes its terms in ascending CSR order, so the bits do not depend on the run, on the split of the rows or on
// the lane mapping below (the noise's row norm is the one reduction across lanes: its order is a function of D alone). include/sibrar_hip.h states the same order; tests/lightgcn_ref.py restates it in numpy. csr_walk.h is not
// used: its walkers enter a sorted row inside a window of columns, and a propagation takes whole rows.
#include "common.h"
#include "philox.h"
#include <cfloat>

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

// what the noisy entry adds to the launch: eps, the key (the halves of seed) and the counter's upper words (the halves of stream_id)
struct GpNoise {
  float eps;
  unsigned int k0, k1, s0, s1;
};

__device__ __forceinline__ float gp_unit(const GpNoise& nz, long r, int block, int word) {
  const uint4 x = philox4x32_10(make_uint4((unsigned int)r, (unsigned int)block, nz.s0, nz.s1), nz.k0, nz.k1);
  return philox_unit(word == 0 ? x.x : word == 1 ? x.y : word == 2 ? x.z : x.w);
}

// A row of 4 D bytes is a gather of latency, not of arithmetic: a full wave on a 64-float row would leave three quarters of its lanes
// without a float4 to load. So a row belongs to a group of G = 2^gshift lanes (G * C * V >= D: lane l of the group owns the V-wide
// chunks l, l + G, ... of the row, C of them), and a wave takes 64 / G consecutive rows. The group reads its neighbours G at a time,
// one per lane (the column, and the scale from the degree in the other side's indptr), and then hands them round by shuffles inside
// the group: GP_UNROLL neighbour rows are loaded before the first of them is added, and the additions follow in CSR order. The groups
// of a wave diverge only in their trip counts; a shuffle's source lane is always in the reader's own group.
//
// NOISE (sbr_graph_propagate_noise_f32) perturbs the finished row in registers. The row's uniforms come in blocks of four columns, one
// Philox call each; the squared norm is summed by the header's rule, which names lanes of a group of G4 = the smallest power of two
// >= ceil(D / 4), 64 at the most: lane l adds the squares of blocks l, l + G4, ... in ascending column order, then the group adds up by
// an xor butterfly from the widest offset down. With float4 chunks G4 is G and the blocks are the lane's own chunks. With single floats
// G >= G4: the lanes below G4 sum their blocks as stated, the others hold +0, and the butterfly over G first adds those zeros (exact)
// and then takes the stated steps, so both paths give the same bits. All lanes of a group share r: they leave together at r >= r1 and
// meet again behind the neighbour loop, so the butterfly reads live lanes only.
template <int V, int C, bool NOISE>
__global__ __launch_bounds__(GP_THREADS) void graph_prop_kernel(const long* __restrict__ u_indptr, const int* __restrict__ u_indices,
                                                                const long* __restrict__ i_indptr, const int* __restrict__ i_indices,
                                                                int n_users, long r0, long r1, const float* __restrict__ x,
                                                                float* __restrict__ y, float* __restrict__ sum, float sum_scale, int D,
                                                                int gshift, GpNoise nz) {
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
  float un[C][V], n_r = 1.f;
  if constexpr (NOISE) {
    float ss = 0.f;
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const int col = (gl + k * G) * 4;
        if (col < D) {
          const uint4 x = philox4x32_10(make_uint4((unsigned int)r, (unsigned int)(col >> 2), nz.s0, nz.s1), nz.k0, nz.k1);
          un[k][0] = philox_unit(x.x); un[k][1] = philox_unit(x.y); un[k][2] = philox_unit(x.z); un[k][3] = philox_unit(x.w);
#pragma unroll
          for (int j = 0; j < 4; ++j) ss = ss + un[k][j] * un[k][j];
        }
      }
    } else {
      const int nb = (D + 3) >> 2;
      int g4 = 1;
      while (g4 < 64 && g4 < nb) g4 <<= 1;
      if (gl < g4) {
        for (int q = gl; q < nb; q += g4) {
          const uint4 x = philox4x32_10(make_uint4((unsigned int)r, (unsigned int)q, nz.s0, nz.s1), nz.k0, nz.k1);
          const unsigned int w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * q + j < D) {
              const float u = philox_unit(w[j]);
              ss = ss + u * u;
            }
        }
      }
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const int col = gl + k * G;
        if (col < D) un[k][0] = gp_unit(nz, r, col >> 2, col & 3);
      }
    }
    for (int off = G >> 1; off > 0; off >>= 1) ss = ss + __shfl_xor(ss, off, 64);
    n_r = fmaxf(sqrtf(ss), 1e-12f);
  }
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int col = (gl + k * G) * V;
    if (col >= D) continue;
    float out[V];
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = s_r * acc[k][j];
    if constexpr (NOISE) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float p = out[j];
        const float sg = p > 0.f ? 1.f : p < 0.f ? -1.f : 0.f;
        if (sg != 0.f) {                                            // a zero stays as it is: a row without neighbours gets no noise
          float t = nz.eps * un[k][j];
          t = t / n_r;
          t = sg * t;
          out[j] = p + t;
        }
      }
    }
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

template <int V, int C, bool NOISE>
static void gp_launch(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users, long r0, long r1,
                      const float* x, float* y, float* sum, float sum_scale, int D, int gshift, const GpNoise& nz, hipStream_t stream) {
  const long rows_per_block = (long)GP_WAVES << (6 - gshift);
  graph_prop_kernel<V, C, NOISE><<<(unsigned)((r1 - r0 + rows_per_block - 1) / rows_per_block), GP_THREADS, 0, stream>>>(
      u_indptr, u_indices, i_indptr, i_indices, n_users, r0, r1, x, y, sum, sum_scale, D, gshift, nz);
}

// both entries: `nz` NULL is the plain propagation
static int gp_run(const char* who, const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users,
                  int n_items, long r0, long r1, const float* x, float* y, float* sum, float sum_scale, int D, const GpNoise* nz,
                  void* stream) {
  SBR_REQUIRE(D >= 1 && D <= GP_D_MAX, "%s: D=%d outside [1, %d]", who, D, GP_D_MAX);
  SBR_REQUIRE(n_users >= 0 && n_users <= GP_DIM_MAX && n_items >= 0 && n_items <= GP_DIM_MAX, "%s: shape [%d, %d] "
              "outside [0, 2^24] x [0, 2^24]: a degree over 2^24 has no exact fp32 form", who, n_users, n_items);
  const long n = (long)n_users + n_items;
  SBR_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= n, "%s: row range [%ld, %ld) outside [0, %ld]", who, r0, r1, n);
  SBR_REQUIRE(!nz || (nz->eps >= 0.f && nz->eps <= FLT_MAX), "%s: eps=%g must be finite and not negative", who, nz ? (double)nz->eps : 0.);
  const long bytes = 4 * n * D;
  SBR_REQUIRE(!(x && y && sbr_overlap(x, bytes, y, bytes)), "%s: x aliases y: a row reads other rows, so the input table cannot be an output",
              who);
  SBR_REQUIRE(!(x && sum && sbr_overlap(x, bytes, sum, bytes)), "%s: x aliases sum: a row reads other rows, so the input table cannot be an "
              "output", who);
  SBR_REQUIRE(!(y && sum && sbr_overlap(y, bytes, sum, bytes)), "%s: y aliases sum: both are written", who);
  if (r0 == r1) return SBR_OK;
  SBR_REQUIRE(u_indptr && i_indptr && x && y, "%s: null operand", who);                               // (a matrix without entries has no indices)
  // float4 chunks where every row of every table starts on a 16-byte boundary, single floats otherwise; the group is the smallest
  // power of two of lanes that covers the row, a wave at the most, and a lane then owns C chunks
  const bool vec = D % 4 == 0 && ((uintptr_t)x | (uintptr_t)y | (uintptr_t)sum) % 16 == 0;
  const int chunks = vec ? D / 4 : D;
  int gshift = 0;
  while (gshift < 6 && (1 << gshift) < chunks) ++gshift;
  const int per_lane = (chunks + (1 << gshift) - 1) >> gshift;
  hipStream_t st = (hipStream_t)stream;
  const GpNoise none = {0.f, 0u, 0u, 0u, 0u};
#define GP_ARGS u_indptr, u_indices, i_indptr, i_indices, n_users, r0, r1, x, y, sum, sum_scale, D, gshift
#define GP_GO(V, C) (nz ? gp_launch<V, C, true>(GP_ARGS, *nz, st) : gp_launch<V, C, false>(GP_ARGS, none, st))
  if (vec) {
    if (per_lane <= 1) GP_GO(4, 1); else GP_GO(4, 2);
  } else {
    if (per_lane <= 1) GP_GO(1, 1); else if (per_lane <= 2) GP_GO(1, 2); else if (per_lane <= 4) GP_GO(1, 4); else GP_GO(1, 8);
  }
#undef GP_GO
#undef GP_ARGS
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}

extern "C" int sbr_graph_propagate_f32(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users,
                                       int n_items, long r0, long r1, const float* x, float* y, float* sum, float sum_scale, int D,
                                       void* stream) {
  return gp_run("sbr_graph_propagate_f32", u_indptr, u_indices, i_indptr, i_indices, n_users, n_items, r0, r1, x, y, sum, sum_scale, D, nullptr,
                stream);
}

extern "C" int sbr_graph_propagate_noise_f32(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices,
                                             int n_users, int n_items, long r0, long r1, const float* x, float* y, float* sum,
                                             float sum_scale, int D, float eps, unsigned long seed, unsigned long stream_id, void* stream) {
  const GpNoise nz = {eps, (unsigned int)seed, (unsigned int)((unsigned long long)seed >> 32), (unsigned int)stream_id,
                      (unsigned int)((unsigned long long)stream_id >> 32)};
  return gp_run("sbr_graph_propagate_noise_f32", u_indptr, u_indices, i_indptr, i_indices, n_users, n_items, r0, r1, x, y, sum, sum_scale, D,
                &nz, stream);
}
