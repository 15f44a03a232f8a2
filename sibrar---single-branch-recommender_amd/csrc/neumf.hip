// NeuMF / NCF (He et al., WWW 2017): the per-pair MLP of a full-catalogue evaluation, without the [users, items, H1] activation.
//   sbr_neumf_score_all     out[u, i] = (accumulate ? out[u, i] : nothing) + (m(u, i) + c) for every user row of A against every item row of Bt
//   sbr_neumf_score_pairs   the same score for a list of (user slot, item slot) pairs
// The first layer is separable, W1 [pm_u ; qm_i] + b1 = A[u] + Bt[i], and both sides come in as small GEMMs' results; what is left per
// pair is z1 = relu(A[u] + Bt[i]), the tail layers z_l = relu(W_l z_{l-1} + b_l), l = 2..L, and m = <w_h, z_L>. Both entries run the one
// device function neumf_tail on registers that hold one pair's z per lane, so a pair has the same bits through either, in any tile, any
// user chunk and any item shard. Plain fp32 fmaf chains in an order that depends on the widths alone, no atomics: valid in deterministic
// mode as it is. include/sibrar_hip.h states the order; tests/neumf_ref.py bounds its error.
#include "common.h"

#define NEUMF_MAX_H 64               // the widest layer (ops.NEUMF_MAX_H)
#define NEUMF_MAX_LAYERS 4           // H1 .. H4 (ops.NEUMF_MAX_LAYERS)
#define NEUMF_WAVES 4                // waves of a workgroup; they share the item tile and the weights and split the users
#define NEUMF_USER_BLOCK 32          // users of one workgroup, a multiple of NEUMF_WAVES * (pairs per lane)
#define NEUMF_LDS_DEFAULT 65536      // the dynamic LDS a launch may ask for without raising the limit
#define NEUMF_MAX_GROUPS (1L << 24)  // workgroups of one launch: HIP refuses more than 2^32 - 1 threads, and a workgroup has 256

struct NeumfDims {
  int L;                             // 1 .. NEUMF_MAX_LAYERS
  int h[NEUMF_MAX_LAYERS];           // H1 .. HL
};

static __host__ __device__ __forceinline__ int neumf_r4(int n) { return (n + 3) & ~3; }

// floats of the packed buffer: W_2 .. W_L row-major [H_l, H_{l-1}], then b_2 .. b_L, then w_h [H_L], then c
static inline long neumf_packed_len(const NeumfDims& d) {
  long n = 0;
  for (int l = 1; l < d.L; ++l) n += (long)d.h[l] * d.h[l - 1] + d.h[l];
  return n + d.h[d.L - 1] + 1;
}
// floats of the LDS image: per tail layer the weights [r4(H_l)][r4(H_{l-1})] and the bias [r4(H_l)], then w_h [r4(H_L)], then c (4 cells);
// the padding is +0, every row starts on a 16-byte boundary
static inline long neumf_lds_len(const NeumfDims& d) {
  long n = 0;
  for (int l = 1; l < d.L; ++l) n += (long)neumf_r4(d.h[l]) * neumf_r4(d.h[l - 1]) + neumf_r4(d.h[l]);
  return n + neumf_r4(d.h[d.L - 1]) + 4;
}

// The workgroup copies the packed buffer into its padded LDS image. The caller puts a barrier behind it.
__device__ __forceinline__ void neumf_stage_tail(const float* __restrict__ tail, const NeumfDims& d, float* __restrict__ lds) {
  const int tid = threadIdx.x, nt = blockDim.x;
  long src_w = 0, src_b = 0;
  for (int l = 1; l < d.L; ++l) src_b += (long)d.h[l] * d.h[l - 1];
  int dst = 0;
  for (int l = 1; l < d.L; ++l) {
    const int hin = d.h[l - 1], hout = d.h[l], cin = neumf_r4(hin), rout = neumf_r4(hout);
    for (int e = tid; e < rout * cin; e += nt) {
      const int j = e / cin, k = e - j * cin;
      lds[dst + e] = (j < hout && k < hin) ? tail[src_w + (long)j * hin + k] : 0.f;
    }
    dst += rout * cin;
    for (int e = tid; e < rout; e += nt) lds[dst + e] = e < hout ? tail[src_b + e] : 0.f;
    dst += rout;
    src_w += (long)hout * hin;
    src_b += hout;
  }
  const int hl = d.h[d.L - 1], rl = neumf_r4(hl);
  for (int e = tid; e < rl; e += nt) lds[dst + e] = e < hl ? tail[src_b + e] : 0.f;
  dst += rl;
  if (tid < 4) lds[dst + tid] = tid == 0 ? tail[src_b + hl] : 0.f;
}

// One lane, U pairs: z[u][0 .. W) holds z1 of pair u, +0 from H1 up. -> m[u] + c.
// Layer l: y_j = relu(chain), the chain being acc = b_l[j]; acc = fmaf(W_l[j][k], z[k], acc) for k = 0, 1, ... ascending. The chain runs to
// the width rounded up to 4: the cells past the width hold a +0 weight and a +0 z, so they add +0 and change no value. Rows past H_l have
// +0 weights and a +0 bias and give the +0 padding of the next layer's z. m = the same chain over w_h from +0. The weights are LDS
// broadcasts (every lane reads the same 16 bytes), each feeding U fmaf; all register indices are compile-time constants, the guards
// on the widths are wave-uniform.
template <int W, int U>
__device__ __forceinline__ void neumf_tail(const float* __restrict__ lds, const NeumfDims& d, float (&z)[U][W], float (&res)[U]) {
#pragma clang fp contract(off)
  int hin = d.h[0];
  const float* p = lds;
  for (int l = 1; l < d.L; ++l) {
    const int hout = d.h[l], cin = neumf_r4(hin), rout = neumf_r4(hout);
    const float* wl = p;
    const float* bl = p + rout * cin;
    p = bl + rout;
    float y[U][W];
#pragma unroll
    for (int j0 = 0; j0 < W; j0 += 4) {
      float acc[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[u][jj] = 0.f;
      if (j0 < hout) {
        const float4 bias = *reinterpret_cast<const float4*>(bl + j0);
        const float bv[4] = {bias.x, bias.y, bias.z, bias.w};
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[u][jj] = bv[jj];
#pragma unroll
        for (int k0 = 0; k0 < W; k0 += 4) {
          if (k0 < hin) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
              const float4 w4 = *reinterpret_cast<const float4*>(wl + (j0 + jj) * cin + k0);
              const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
              for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u][jj] = fmaf(wv[kk], z[u][k0 + kk], acc[u][jj]);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[u][jj] = sbr_relu(acc[u][jj]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) y[u][j0 + jj] = acc[u][jj];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < W; ++k) z[u][k] = y[u][k];
    hin = hout;
  }
  float m[U];
#pragma unroll
  for (int u = 0; u < U; ++u) m[u] = 0.f;
#pragma unroll
  for (int k0 = 0; k0 < W; k0 += 4) {
    if (k0 < hin) {
      const float4 w4 = *reinterpret_cast<const float4*>(p + k0);
      const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int u = 0; u < U; ++u) m[u] = fmaf(wv[kk], z[u][k0 + kk], m[u]);
    }
  }
  const float c = p[neumf_r4(hin)];
#pragma unroll
  for (int u = 0; u < U; ++u) res[u] = m[u] + c;
}

// Workgroup = (a tile of 64 items) x (a block of NEUMF_USER_BLOCK users). A lane owns one item and keeps its Bt row in registers. The
// block's A rows are staged in LDS behind the weights, +0 past H1 and past Bu, and read as broadcasts. The four waves share the tile and
// take U users at a time, wave w the users w U, w U + 1, ..., then 4 U further on. Lanes past I and users past Bu compute on staged
// zeros and write nothing.
template <int W, int U>
__global__ __launch_bounds__(64 * NEUMF_WAVES) void neumf_score_all_kernel(const float* __restrict__ A, long stride_a,
                                                                           const float* __restrict__ Bt, long stride_b,
                                                                           const float* __restrict__ tail, NeumfDims d, int tail_cells,
                                                                           float* out, long stride_o, int Bu, int I, int n_item_tiles,
                                                                           int accumulate) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float neumf_lds[];
  const int h1 = d.h[0], c1 = neumf_r4(h1);
  const int tile = (int)(blockIdx.x % (unsigned)n_item_tiles), ublock = (int)(blockIdx.x / (unsigned)n_item_tiles);
  const long u_begin = (long)ublock * NEUMF_USER_BLOCK;
  const long u_end = u_begin + NEUMF_USER_BLOCK < Bu ? u_begin + NEUMF_USER_BLOCK : (long)Bu;
  float* a_lds = neumf_lds + tail_cells;
  neumf_stage_tail(tail, d, neumf_lds);
  for (int e = threadIdx.x; e < NEUMF_USER_BLOCK * c1; e += 64 * NEUMF_WAVES) {
    const int r = e / c1, k = e - r * c1;
    a_lds[e] = (u_begin + r < u_end && k < h1) ? A[(u_begin + r) * stride_a + k] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = (int)(threadIdx.x >> 6);
  const long item = (long)tile * 64 + lane;
  const bool item_ok = item < I;
  const float* b_row = Bt + (item_ok ? item : (long)I - 1) * stride_b;      // a lane past I reads the last row and writes nothing
  float b[W];
#pragma unroll
  for (int k0 = 0; k0 < W; k0 += 4) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) b[k0 + kk] = 0.f;
    if (k0 < h1) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int k = k0 + kk;
        const float v = b_row[k < h1 ? k : h1 - 1];
        b[k] = k < h1 ? v : 0.f;
      }
    }
  }
  for (int r0 = wave * U; u_begin + r0 < u_end; r0 += NEUMF_WAVES * U) {
    float z[U][W], res[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* a = a_lds + (r0 + u) * c1;                 // r0 + u < NEUMF_USER_BLOCK: the block is a multiple of 4 U
#pragma unroll
      for (int k0 = 0; k0 < W; k0 += 4) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) z[u][k0 + kk] = 0.f;
        if (k0 < h1) {
          const float4 a4 = *reinterpret_cast<const float4*>(a + k0);
          const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) z[u][k0 + kk] = sbr_relu(av[kk] + b[k0 + kk]);
        }
      }
    }
    neumf_tail<W, U>(neumf_lds, d, z, res);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u_begin + r0 + u < u_end && item_ok) {
        float* o = out + (u_begin + r0 + u) * stride_o + item;
        *o = accumulate ? *o + res[u] : res[u];
      }
    }
  }
}

// The pair list: a workgroup owns 64 * NEUMF_WAVES * U consecutive pairs, thread t the pairs base + t, base + t + 256, ... . Both rows of
// a pair are per-lane reads. A slot outside its operand reads nothing and gives a NaN.
template <int W, int U>
__global__ __launch_bounds__(64 * NEUMF_WAVES) void neumf_score_pairs_kernel(const float* __restrict__ A, long stride_a, int Bu,
                                                                             const float* __restrict__ Bt, long stride_b, int I,
                                                                             const int* __restrict__ u_slot, const int* __restrict__ i_slot,
                                                                             const float* __restrict__ tail, NeumfDims d, float* out, long R,
                                                                             int accumulate) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float neumf_lds[];
  neumf_stage_tail(tail, d, neumf_lds);
  __syncthreads();
  const int h1 = d.h[0];
  const long base = (long)blockIdx.x * (64 * NEUMF_WAVES * U) + threadIdx.x;
  float z[U][W], res[U];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long r = base + (long)u * (64 * NEUMF_WAVES);
    ok[u] = false;
    long us = 0, is = 0;
    if (r < R) {
      us = u_slot[r];
      is = i_slot[r];
      ok[u] = us >= 0 && us < Bu && is >= 0 && is < I;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      z[u][k] = 0.f;
      if (k < h1 && ok[u]) z[u][k] = sbr_relu(A[us * stride_a + k] + Bt[is * stride_b + k]);
    }
  }
  neumf_tail<W, U>(neumf_lds, d, z, res);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long r = base + (long)u * (64 * NEUMF_WAVES);
    if (r < R) {
      const float v = ok[u] ? res[u] : __builtin_nanf("");
      out[r] = accumulate ? out[r] + v : v;
    }
  }
}

static int neumf_dims(const char* who, int n_layers, int h1, int h2, int h3, int h4, long tail_len, NeumfDims* d, size_t* lds_bytes) {
  SBR_REQUIRE(n_layers >= 1 && n_layers <= NEUMF_MAX_LAYERS, "%s: %d layers outside [1, %d]", who, n_layers, NEUMF_MAX_LAYERS);
  const int h[NEUMF_MAX_LAYERS] = {h1, h2, h3, h4};
  d->L = n_layers;
  for (int l = 0; l < NEUMF_MAX_LAYERS; ++l) {
    d->h[l] = l < n_layers ? h[l] : 0;
    SBR_REQUIRE(l >= n_layers || (h[l] >= 1 && h[l] <= NEUMF_MAX_H), "%s: layer %d has width %d outside [1, %d]", who, l + 1, h[l],
                NEUMF_MAX_H);
  }
  SBR_REQUIRE(tail_len == neumf_packed_len(*d), "%s: the packed tail holds %ld floats, these widths need %ld", who, tail_len,
              neumf_packed_len(*d));
  *lds_bytes = (size_t)neumf_lds_len(*d) * sizeof(float);
  SBR_REQUIRE(*lds_bytes <= NEUMF_LDS_DEFAULT, "%s: the weights need %zu bytes of LDS, over %d", who, *lds_bytes, NEUMF_LDS_DEFAULT);
  return SBR_OK;
}

static inline int neumf_max_width(const NeumfDims& d) {
  int w = 0;
  for (int l = 0; l < d.L; ++l) w = d.h[l] > w ? d.h[l] : w;
  return w;
}

// (register width, pairs per lane) by the widest layer: the pairs a lane holds divide the LDS reads per fmaf, the registers bound them
#define NEUMF_DISPATCH(GO)                \
  do {                                    \
    const int mw__ = neumf_max_width(d);  \
    if (mw__ <= 8) GO(8, 4);              \
    else if (mw__ <= 16) GO(16, 4);       \
    else if (mw__ <= 32) GO(32, 2);       \
    else GO(64, 1);                       \
  } while (0)

static inline int neumf_pairs_per_lane(const NeumfDims& d) {
  const int mw = neumf_max_width(d);
  return mw <= 16 ? 4 : mw <= 32 ? 2 : 1;
}

extern "C" int sbr_neumf_score_all(const float* A, long stride_a, const float* Bt, long stride_b, const float* tail, long tail_len,
                                   int n_layers, int h1, int h2, int h3, int h4, float* out, long stride_o, int Bu, int I,
                                   int accumulate, void* stream) {
  const char* who = "sbr_neumf_score_all";
  NeumfDims d;
  size_t lds_bytes = 0;
  if (int rc = neumf_dims(who, n_layers, h1, h2, h3, h4, tail_len, &d, &lds_bytes)) return rc;
  SBR_REQUIRE(Bu >= 0 && I >= 0, "%s: negative shape (Bu=%d, I=%d)", who, Bu, I);
  if (Bu == 0 || I == 0) return SBR_OK;
  SBR_REQUIRE(A && Bt && tail && out, "%s: null operand", who);
  SBR_REQUIRE(stride_a >= h1 && stride_b >= h1 && stride_o >= I, "%s: row strides (%ld, %ld, %ld) below the row lengths (%d, %d, %d)", who,
              stride_a, stride_b, stride_o, h1, h1, I);
  const long n_tiles = ((long)I + 63) / 64, n_ublocks = ((long)Bu + NEUMF_USER_BLOCK - 1) / NEUMF_USER_BLOCK;
  SBR_REQUIRE(n_tiles * n_ublocks <= NEUMF_MAX_GROUPS, "%s: %ld workgroups, over 2^24: score the users in chunks", who, n_tiles * n_ublocks);
  const size_t all_bytes = lds_bytes + sizeof(float) * NEUMF_USER_BLOCK * neumf_r4(h1);
  SBR_REQUIRE(all_bytes <= NEUMF_LDS_DEFAULT, "%s: the weights and the user block need %zu bytes of LDS, over %d", who, all_bytes,
              NEUMF_LDS_DEFAULT);
#define NEUMF_GO(WW, UU)                                                                                                     \
  neumf_score_all_kernel<WW, UU><<<(unsigned)(n_tiles * n_ublocks), 64 * NEUMF_WAVES, all_bytes, (hipStream_t)stream>>>(     \
      A, stride_a, Bt, stride_b, tail, d, (int)(lds_bytes / sizeof(float)), out, stride_o, Bu, I, (int)n_tiles, accumulate)
  NEUMF_DISPATCH(NEUMF_GO);
#undef NEUMF_GO
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}

extern "C" int sbr_neumf_score_pairs(const float* A, long stride_a, int Bu, const float* Bt, long stride_b, int I, const int* u_slot,
                                     const int* i_slot, const float* tail, long tail_len, int n_layers, int h1, int h2, int h3, int h4,
                                     float* out, long R, int accumulate, void* stream) {
  const char* who = "sbr_neumf_score_pairs";
  NeumfDims d;
  size_t lds_bytes = 0;
  if (int rc = neumf_dims(who, n_layers, h1, h2, h3, h4, tail_len, &d, &lds_bytes)) return rc;
  SBR_REQUIRE(Bu >= 0 && I >= 0 && R >= 0, "%s: negative shape (Bu=%d, I=%d, R=%ld)", who, Bu, I, R);
  if (R == 0) return SBR_OK;
  SBR_REQUIRE(A && Bt && tail && out && u_slot && i_slot, "%s: null operand", who);
  SBR_REQUIRE(stride_a >= h1 && stride_b >= h1, "%s: row strides (%ld, %ld) below the row length %d", who, stride_a, stride_b, h1);
  const long per_block = 64L * NEUMF_WAVES * neumf_pairs_per_lane(d), n_blocks = (R + per_block - 1) / per_block;
  SBR_REQUIRE(n_blocks <= NEUMF_MAX_GROUPS, "%s: %ld workgroups, over 2^24: score the pairs in chunks", who, n_blocks);
#define NEUMF_GO(WW, UU)                                                                                               \
  neumf_score_pairs_kernel<WW, UU><<<(unsigned)n_blocks, 64 * NEUMF_WAVES, lds_bytes, (hipStream_t)stream>>>(          \
      A, stride_a, Bu, Bt, stride_b, I, u_slot, i_slot, tail, d, out, R, accumulate)
  NEUMF_DISPATCH(NEUMF_GO);
#undef NEUMF_GO
  SBR_CHECK_LAUNCH(who);
  return SBR_OK;
}
