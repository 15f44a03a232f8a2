// NGCF's layer (Wang et al., SIGIR 2019) over the joint row space of the bipartite user-item graph, one launch per layer and direction:
//   sbr_ngcf_layer_fwd  s = A^ x (graph_prop.hip's gather, bit for bit), a = s + x, b = s * x, z = a W1 + b W2 + bias,
//                       h = dropout(LeakyReLU(z)), out = h / max(|h|, 1e-12) written into a column slice of a wider table
//   sbr_ngcf_layer_bwd  dz from the gradients of out and h; ds = da + db * x and dx_direct = da + db * s with da = dz W1^T, db = dz W2^T;
//                       dW1 = a^T dz, dW2 = b^T dz, dbias = colsum(dz)
// A workgroup owns 64 rows. It gathers s for them with the lane-group scheme of graph_prop.hip (a row belongs to G lanes, the
// neighbours are handed round by shuffles, GP_UNROLL rows in flight, the additions in CSR order), but into LDS instead of memory; the
// products run from there through the 64 x 64 tile skeleton (tile64_f32.h) with 32-row chunks of W1 and W2 staged in LDS, and the
// epilogue stays in registers. s, a and b never reach memory.
//
// What the forward pass saves for the backward pass: nothing of its own. The backward pass takes x (the layer's input) and h (its
// output, the next layer's input, which the caller keeps anyway) and recomputes the gather, the Philox mask and the row norm; the norm
// is summed in the forward order, so it is the forward's, bit for bit.
//
// Widths: 1 <= Din, Dout <= NG_W_MAX = 128. At the cap the forward kernel holds a and b (2 x 128 x 68 floats) and one chunk in
// 78,336 bytes of LDS, the backward kernel s and x and three chunks in 95,744 bytes; 256 would need more than the 160 KiB of a CU
// in the backward pass, so the cap stays where the issue put it.
//
// Orders (include/sibrar_hip.h states them, tests/ngcf_ref.py restates the forward in numpy). z[j]: one accumulator from +0, fmaf over
// k ascending of a[k] W1[k][j], then of b[k] W2[k][j], then one addition of the bias: a function of nothing but (Din, Dout); rows of
// zeros that pad Din to a multiple of 32 add +0 * +0, which changes no bit. The squared norm: 16 partial sums, partial l over the
// columns j with (j / 4) % 16 == l ascending, then an xor butterfly over the offsets 1, 2, 4, 8. The gather's loop is a copy of
// graph_prop.hip's, not shared code: there it ends in a store and an early return, here in LDS and a barrier, and the kernel that
// every graph model runs is left exactly as it was.
#include "tile64_f32.h"
#include "philox.h"
#include <cfloat>

#define NG_THREADS 256
#define NG_UNROLL 8                  // neighbour rows in flight per lane group, as GP_UNROLL
#define NG_W_MAX 128
#define NG_DIM_MAX (1 << 24)
constexpr int NG_TILE = T64_T * T64_LD;          // floats of one [64][T64_LD] LDS tile
constexpr int NG_CHUNK = T64_KC * T64_LD;        // floats of one staged chunk

struct NgGraph {
  const long* u_indptr; const int* u_indices; const long* i_indptr; const int* i_indices;
  int n_users;
};
// the dropout of a launch: rate, 1 / (1 - p), the key (the halves of seed) and the counter's upper words (the halves of stream_id)
struct NgDrop {
  float p, inv_keep;
  unsigned int k0, k1, s0, s1;
};

__device__ __forceinline__ float ng_scale(long d) { return d > 0 ? 1.0f / sqrtf((float)d) : 0.f; }     // gp_scale of graph_prop.hip

template <int V> struct NgVec;
template <> struct NgVec<4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
};
template <> struct NgVec<1> {
  static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
};

// s of the tile's 64 rows j0 .. j0 + 63, 256 >> gshift rows at a time (2 <= gshift <= 6): put(rl, r, live, col, s[V]) is called once
// for every row rl of the tile and every V-wide chunk of columns below D. A row at or past r1 is not live: it reads nothing and its s
// is +0. All lanes of a group share the row, so the shuffles read lanes that run the same trip counts.
template <int V, int C, class F>
__device__ __forceinline__ void ng_gather(const NgGraph& g, long j0, long r1, const float* __restrict__ x, int D, int gshift, int t, F put) {
#pragma clang fp contract(off)
  const int G = 1 << gshift;
  const int lane = t & 63, gl = lane & (G - 1), gbase = lane - gl;
  const int per_pass = NG_THREADS >> gshift;
  for (int rl0 = 0; rl0 < T64_T; rl0 += per_pass) {
    const int rl = rl0 + (t >> gshift);
    const long r = j0 + rl;
    const bool live = r < r1;
    const bool user = r < g.n_users;
    const long* indptr = user ? g.u_indptr : g.i_indptr;
    const int* indices = user ? g.u_indices : g.i_indices;
    const long* o_indptr = user ? g.i_indptr : g.u_indptr;
    const long local = user ? r : r - g.n_users;
    const long c_base = user ? g.n_users : 0;
    long beg = 0, end = 0;
    if (live) { beg = indptr[local]; end = indptr[local + 1]; }
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
        my_s = ng_scale(o_indptr[my_c + 1] - o_indptr[my_c]);
      }
      for (int e0 = 0; e0 < n_e; e0 += NG_UNROLL) {
        float v[NG_UNROLL][C][V], s[NG_UNROLL];
#pragma unroll
        for (int u = 0; u < NG_UNROLL; ++u) {
          if (e0 + u < n_e) {
            const float* xr = x + (c_base + (long)__shfl(my_c, gbase + e0 + u, 64)) * D;
            s[u] = __shfl(my_s, gbase + e0 + u, 64);
#pragma unroll
            for (int k = 0; k < C; ++k) {
              const int col = (gl + k * G) * V;
              if (col < D) NgVec<V>::load(xr + col, v[u][k]);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < NG_UNROLL; ++u) {
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
    const float s_r = ng_scale(end - beg);
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const int col = (gl + k * G) * V;
      if (col >= D) continue;
      float out[V];
#pragma unroll
      for (int j = 0; j < V; ++j) out[j] = s_r * acc[k][j];
      put(rl, r, live, col, out);
    }
  }
}

// keep[c] of the four columns of block `block` of row r: u >= p; one Philox call
__device__ __forceinline__ void ng_keep(const NgDrop& dr, long r, int block, bool (&keep)[4]) {
  const uint4 w = philox4x32_10(make_uint4((unsigned int)r, (unsigned int)block, dr.s0, dr.s1), dr.k0, dr.k1);
  keep[0] = philox_unit(w.x) >= dr.p; keep[1] = philox_unit(w.y) >= dr.p;
  keep[2] = philox_unit(w.z) >= dr.p; keep[3] = philox_unit(w.w) >= dr.p;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// LDS: La [KP][T64_LD] and Lb [KP][T64_LD], K-major (KP = Din rounded up to the chunk), then one chunk of W
template <int V, int C, int NPT>
__global__ __launch_bounds__(NG_THREADS) void ngcf_fwd_kernel(NgGraph g, long r0, long r1, const float* __restrict__ x,
                                                               const float* __restrict__ W1, const float* __restrict__ W2,
                                                               const float* __restrict__ bias, float slope, NgDrop dr, float* __restrict__ h,
                                                               float* __restrict__ outn, long out_ld, int Din, int Dout, int gshift) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float ng_lds[];
  const int KP = (Din + T64_KC - 1) & ~(T64_KC - 1);
  float* La = ng_lds;
  float* Lb = La + KP * T64_LD;
  float* Bs = Lb + KP * T64_LD;
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4, bc = t & 63, bk = t >> 6;
  const long j0 = r0 + (long)blockIdx.x * T64_T;
  for (int e = t; e < (KP - Din) * T64_T; e += NG_THREADS) {       // the rows that pad Din to the chunk
    const int at = (Din + (e >> 6)) * T64_LD + (e & 63);
    La[at] = 0.f; Lb[at] = 0.f;
  }
  ng_gather<V, C>(g, j0, r1, x, Din, gshift, t, [&](int rl, long r, bool live, int col, const float (&s)[V]) {
    float xv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) xv[j] = 0.f;
    if (live) NgVec<V>::load(x + r * Din + col, xv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      La[(col + j) * T64_LD + rl] = s[j] + xv[j];
      Lb[(col + j) * T64_LD + rl] = s[j] * xv[j];
    }
  });
  __syncthreads();
  float acc[NPT][4][4];
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt) {
    t64_zero(acc[pt]);
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const float* W = w ? W2 : W1;
      const float* L = w ? Lb : La;
      for (int k0 = 0; k0 < KP; k0 += T64_KC) {
        t64_stage_chunk<false>(Bs, W, nullptr, k0, Din, pt, Dout, bc, bk);
        __syncthreads();
        t64_mma(L + k0 * T64_LD, Bs, rg, cg, acc[pt]);
        __syncthreads();
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long r = j0 + 4 * rg + i;
    float hv[NPT][4], q = 0.f;
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
      bool keep[4] = {true, true, true, true};
      if (dr.p > 0.f && pt * T64_T + 4 * cg < Dout) ng_keep(dr, r, pt * 16 + cg, keep);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = pt * T64_T + 4 * cg + c;
        float v = 0.f;
        if (j < Dout) {
          const float z = acc[pt][i][c] + bias[j];
          v = z > 0.f ? z : slope * z;
          if (dr.p > 0.f) v = keep[c] ? v * dr.inv_keep : 0.f;
        }
        hv[pt][c] = v;
        q = q + v * v;
      }
    }
    q = t64_row_sum(q);
    const float nrm = fmaxf(sqrtf(q), T64_EPS);
    if (r >= r1) continue;
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = pt * T64_T + 4 * cg + c;
        if (j < Dout) {
          h[r * Dout + j] = hv[pt][c];
          outn[r * out_ld + j] = hv[pt][c] / nrm;
        }
      }
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// LDS: Ls [KT][64][T64_LD] and Lx [KT][64][T64_LD], row-major (they become a and b in place before the weight products), then three
// chunks. part: [nb][Din Dout] of dW1, [nb][Din Dout] of dW2, [nb][Dout] of dbias, one slice per workgroup, folded in workgroup order.
template <int V, int C, int NPT, int KT>
__global__ __launch_bounds__(NG_THREADS) void ngcf_bwd_kernel(NgGraph g, long r0, long r1, const float* __restrict__ x,
                                                               const float* __restrict__ W1, const float* __restrict__ W2, float slope,
                                                               NgDrop dr, const float* __restrict__ h, const float* __restrict__ g_out,
                                                               long out_ld, const float* __restrict__ g_h, float* __restrict__ ds,
                                                               float* __restrict__ dxd, float* __restrict__ part, int n_tiles, int Din,
                                                               int Dout, int gshift) {
  extern __shared__ __align__(16) float ng_lds[];
  __shared__ float s_wc[4][T64_T];
  __shared__ float s_col[NPT * T64_T];
  float* Ls = ng_lds;
  float* Lx = Ls + KT * NG_TILE;
  float* As = Lx + KT * NG_TILE;
  float* B1 = As + NG_CHUNK;
  float* B2 = B1 + NG_CHUNK;
  const int t = threadIdx.x, cg = t & 15, rg = t >> 4, sk = t & 31, sr = t >> 5;
  const long DD = (long)Din * Dout;
  float* my_w1 = part + blockIdx.x * DD;
  float* my_w2 = part + (gridDim.x + (long)blockIdx.x) * DD;
  float* my_b = part + 2 * gridDim.x * DD + (long)blockIdx.x * Dout;
  if (t < NPT * T64_T) s_col[t] = 0.f;
  bool first = true;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, first = false) {
    const long j0 = r0 + (long)tile * T64_T;
    for (int e = t; e < (KT * T64_T - Din) * T64_T; e += NG_THREADS) {      // the columns that pad Din to the tile
      const int col = Din + e / T64_T, at = (col >> 6) * NG_TILE + (e % T64_T) * T64_LD + (col & 63);
      Ls[at] = 0.f; Lx[at] = 0.f;
    }
    ng_gather<V, C>(g, j0, r1, x, Din, gshift, t, [&](int rl, long r, bool live, int col, const float (&s)[V]) {
      float xv[V];
#pragma unroll
      for (int j = 0; j < V; ++j) xv[j] = 0.f;
      if (live) NgVec<V>::load(x + r * Din + col, xv);
      const int at = (col >> 6) * NG_TILE + rl * T64_LD + (col & 63);
#pragma unroll
      for (int j = 0; j < V; ++j) { Ls[at + j] = s[j]; Lx[at + j] = xv[j]; }
    });
    __syncthreads();
    // dz: undo the normalisation, the dropout and the LeakyReLU; zero for the rows past r1 and the columns past Dout
    float dz[NPT][4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long r = j0 + 4 * rg + i;
      const bool live = r < r1;
      float hv[NPT][4], go[NPT][4], q = 0.f;
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = pt * T64_T + 4 * cg + c;
          const bool in = live && j < Dout;
          hv[pt][c] = in ? h[r * Dout + j] : 0.f;
          go[pt][c] = in ? g_out[r * out_ld + j] : 0.f;
          {
#pragma clang fp contract(off)
            q = q + hv[pt][c] * hv[pt][c];                             // the forward's order: the same norm, bit for bit
          }
        }
      q = t64_row_sum(q);
      float nrm, flag;
      t64_stats(q, nrm, flag);
      float dot = 0.f;
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int c = 0; c < 4; ++c) dot = fmaf(go[pt][c], hv[pt][c] / nrm, dot);
      dot = t64_row_sum(dot) * flag;
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        bool keep[4] = {true, true, true, true};
        if (dr.p > 0.f && pt * T64_T + 4 * cg < Dout) ng_keep(dr, r, pt * 16 + cg, keep);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = pt * T64_T + 4 * cg + c;
          float d = 0.f;
          if (live && j < Dout) {
            d = (go[pt][c] - (hv[pt][c] / nrm) * dot) / nrm;
            if (g_h) d += g_h[r * Dout + j];
            if (dr.p > 0.f) d = keep[c] ? d * dr.inv_keep : 0.f;
            d = hv[pt][c] > 0.f ? d : slope * d;                       // slope > 0: a kept h has the sign of z
          }
          dz[pt][i][c] = d;
        }
      }
    }
    // da = dz W1^T, db = dz W2^T, one 64-wide tile of Din at a time; ds and dx_direct from them and the s and x of LDS
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      float da[4][4], db[4][4];
      t64_zero(da);
      t64_zero(db);
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int c0 = pt * T64_T + half * T64_KC;
          if (c0 < Dout) {                                             // the same for every thread
            t64_stage_regs_t(As, dz[pt], half, rg, cg);
            t64_stage_tile_t(B1, W1, kt, Din, c0 + sk, Dout, sk, sr);
            t64_stage_tile_t(B2, W2, kt, Din, c0 + sk, Dout, sk, sr);
            __syncthreads();
            t64_mma(As, B1, rg, cg, da);
            t64_mma(As, B2, rg, cg, db);
            __syncthreads();
          }
        }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long r = j0 + 4 * rg + i;
        if (r >= r1) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = kt * T64_T + 4 * cg + c;
          if (k < Din) {
            const int at = kt * NG_TILE + (4 * rg + i) * T64_LD + 4 * cg + c;
            ds[r * Din + k] = fmaf(db[i][c], Lx[at], da[i][c]);
            dxd[r * Din + k] = fmaf(db[i][c], Ls[at], da[i][c]);
          }
        }
      }
    }
    __syncthreads();
    for (int e = t; e < KT * T64_T * T64_T; e += NG_THREADS) {         // (s, x) -> (a, b) in place
      const int at = (e >> 6) * T64_LD + (e & 63);
      const float sv = Ls[at], xv = Lx[at];
      Ls[at] = sv + xv;
      Lx[at] = sv * xv;
    }
    __syncthreads();
    // dW1 += a^T dz, dW2 += b^T dz over this tile's rows, into the workgroup's own partials
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        float w1[4][4], w2[4][4];
        t64_zero(w1);
        t64_zero(w2);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          t64_stage_regs(B1, dz[pt], half, rg, cg);
          __syncthreads();
          t64_mma(Ls + kt * NG_TILE + half * NG_CHUNK, B1, rg, cg, w1);
          t64_mma(Lx + kt * NG_TILE + half * NG_CHUNK, B1, rg, cg, w2);
          __syncthreads();
        }
        t64_part_add(my_w1, w1, kt, Din, pt, Dout, t, first);
        t64_part_add(my_w2, w2, kt, Din, pt, Dout, t, first);
      }
    t64_col_sums<NPT>(s_wc, s_col, Dout, t, [&](int pt, int c) { return (dz[pt][0][c] + dz[pt][1][c]) + (dz[pt][2][c] + dz[pt][3][c]); });
  }
  __syncthreads();
  if (t < Dout) my_b[t] = s_col[t];
}

struct NgFoldEpi {
  static constexpr bool kColumnSums = false;
  __device__ __forceinline__ float operator()(long, int, float s, float) const { return s; }
};

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static inline size_t ng_fwd_lds(int Din) { return (size_t)(2 * ((Din + T64_KC - 1) & ~(T64_KC - 1)) * T64_LD + NG_CHUNK) * sizeof(float); }
static inline size_t ng_bwd_lds(int Din) { return (size_t)(2 * t64_tiles(Din) * NG_TILE + 3 * NG_CHUNK) * sizeof(float); }
static inline int ng_splits(long R, int Din, int Dout) { return t64_splits(R, 2L * Din * Dout + Dout); }
static inline size_t ng_bwd_ws_bytes(long R, int Din, int Dout) { return (size_t)ng_splits(R, Din, Dout) * (2 * (size_t)Din * Dout + Dout) * sizeof(float); }

// the lane group of the gather: float4 chunks where the rows of x start on a 16-byte boundary, single floats otherwise; at least four
// lanes (256 threads cover at most the tile's 64 rows in a pass), a wave at the most
static void ng_group(const float* x, int Din, bool* vec, int* gshift, int* per_lane) {
  *vec = Din % 4 == 0 && (uintptr_t)x % 16 == 0;
  const int chunks = *vec ? Din / 4 : Din;
  int s = 2;
  while (s < 6 && (1 << s) < chunks) ++s;
  *gshift = s;
  *per_lane = (chunks + (1 << s) - 1) >> s;
}

struct NgArgs {
  const char* who;
  NgGraph g;
  long r0, r1, n;
  int Din, Dout;
  float slope;
  NgDrop dr;
};

// the checks both entries share; the row range and the graph as sbr_graph_propagate_f32 has them
static int ng_check(NgArgs* a, const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users, int n_items,
                    long r0, long r1, int Din, int Dout, float slope, float p, unsigned long seed, unsigned long stream_id) {
  const char* who = a->who;
  SBR_REQUIRE(Din >= 1 && Din <= NG_W_MAX && Dout >= 1 && Dout <= NG_W_MAX, "%s: widths Din=%d, Dout=%d outside [1, %d]", who, Din, Dout,
              NG_W_MAX);
  SBR_REQUIRE(n_users >= 0 && n_users <= NG_DIM_MAX && n_items >= 0 && n_items <= NG_DIM_MAX, "%s: shape [%d, %d] "
              "outside [0, 2^24] x [0, 2^24]: a degree over 2^24 has no exact fp32 form", who, n_users, n_items);
  const long n = (long)n_users + n_items;
  SBR_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= n, "%s: row range [%ld, %ld) outside [0, %ld]", who, r0, r1, n);
  SBR_REQUIRE(slope > 0.f && slope <= 1.f, "%s: slope=%g outside (0, 1]", who, (double)slope);
  SBR_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout rate p=%g outside [0, 1)", who, (double)p);
  a->g = NgGraph{u_indptr, u_indices, i_indptr, i_indices, n_users};
  a->r0 = r0; a->r1 = r1; a->n = n; a->Din = Din; a->Dout = Dout; a->slope = slope;
  a->dr = NgDrop{p, 1.0f / (1.0f - p), (unsigned int)seed, (unsigned int)((unsigned long long)seed >> 32), (unsigned int)stream_id,
                 (unsigned int)((unsigned long long)stream_id >> 32)};
  return SBR_OK;
}

struct NgSpan { const char* name; const void* p; long bytes; bool written; };
// no written table may meet any other table
static int ng_disjoint(const char* who, const NgSpan* s, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if ((s[i].written || s[j].written) && s[i].p && s[j].p && s[i].bytes > 0 && s[j].bytes > 0)
        SBR_REQUIRE(!sbr_overlap(s[i].p, s[i].bytes, s[j].p, s[j].bytes), "%s: %s aliases %s", who, s[i].name, s[j].name);
  return SBR_OK;
}

template <int V, int C, int NPT>
static int ng_fwd_launch(const NgArgs& a, const float* x, const float* W1, const float* W2, const float* bias, float* h, float* out, long out_ld,
                         int gshift, hipStream_t st) {
  static SbrLdsSlot slot;
  const size_t lds = ng_fwd_lds(a.Din);
  if (int rc = sbr_raise_lds(a.who, (const void*)ngcf_fwd_kernel<V, C, NPT>, &slot, lds)) return rc;
  ngcf_fwd_kernel<V, C, NPT><<<t64_tiles(a.r1 - a.r0), NG_THREADS, lds, st>>>(a.g, a.r0, a.r1, x, W1, W2, bias, a.slope, a.dr, h, out, out_ld,
                                                                             a.Din, a.Dout, gshift);
  return SBR_OK;
}

extern "C" int sbr_ngcf_layer_fwd(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users,
                                  int n_items, long r0, long r1, const float* x, int Din, const float* W1, const float* W2, const float* bias,
                                  int Dout, float slope, float p, unsigned long seed, unsigned long stream_id, float* h, float* out,
                                  long out_ld, void* stream) {
  NgArgs a;
  a.who = "sbr_ngcf_layer_fwd";
  if (int rc = ng_check(&a, u_indptr, u_indices, i_indptr, i_indices, n_users, n_items, r0, r1, Din, Dout, slope, p, seed, stream_id)) return rc;
  SBR_REQUIRE(out_ld >= Dout, "%s: out_ld=%ld below Dout=%d", a.who, out_ld, Dout);
  const long wb = 4L * Din * Dout;
  const NgSpan spans[] = {{"x", x, 4 * a.n * Din, false}, {"W1", W1, wb, false}, {"W2", W2, wb, false}, {"bias", bias, 4L * Dout, false},
                          {"h", h, 4 * a.n * Dout, true}, {"out", out, a.n > 0 ? 4 * ((a.n - 1) * out_ld + Dout) : 0, true}};
  if (int rc = ng_disjoint(a.who, spans, 6)) return rc;
  if (r0 == r1) return SBR_OK;
  SBR_REQUIRE(u_indptr && i_indptr && x && W1 && W2 && bias && h && out, "%s: null operand", a.who);        // (a matrix without entries has no indices)
  bool vec;
  int gshift, per_lane;
  ng_group(x, Din, &vec, &gshift, &per_lane);
  hipStream_t st = (hipStream_t)stream;
  int rc = SBR_OK;
#define NG_GO(V, C) (Dout <= T64_T ? ng_fwd_launch<V, C, 1>(a, x, W1, W2, bias, h, out, out_ld, gshift, st) \
                                   : ng_fwd_launch<V, C, 2>(a, x, W1, W2, bias, h, out, out_ld, gshift, st))
  if (vec) rc = NG_GO(4, 1);
  else if (per_lane <= 1) rc = NG_GO(1, 1);
  else rc = NG_GO(1, 2);
#undef NG_GO
  if (rc) return rc;
  SBR_CHECK_LAUNCH(a.who);
  return SBR_OK;
}

extern "C" long sbr_ngcf_layer_bwd_workspace(long n_rows, int Din, int Dout) {
  if (n_rows <= 0 || Din < 1 || Din > NG_W_MAX || Dout < 1 || Dout > NG_W_MAX) return 0;
  return (long)ng_bwd_ws_bytes(n_rows, Din, Dout);
}

template <int V, int C, int NPT, int KT>
static int ng_bwd_launch(const NgArgs& a, const float* x, const float* W1, const float* W2, const float* h, const float* g_out, long out_ld,
                         const float* g_h, float* ds, float* dxd, float* part, int nb, int gshift, hipStream_t st) {
  static SbrLdsSlot slot;
  const size_t lds = ng_bwd_lds(a.Din);
  if (int rc = sbr_raise_lds(a.who, (const void*)ngcf_bwd_kernel<V, C, NPT, KT>, &slot, lds)) return rc;
  ngcf_bwd_kernel<V, C, NPT, KT><<<nb, NG_THREADS, lds, st>>>(a.g, a.r0, a.r1, x, W1, W2, a.slope, a.dr, h, g_out, out_ld, g_h, ds, dxd, part,
                                                            t64_tiles(a.r1 - a.r0), a.Din, a.Dout, gshift);
  return SBR_OK;
}

extern "C" int sbr_ngcf_layer_bwd(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users,
                                  int n_items, long r0, long r1, const float* x, int Din, const float* W1, const float* W2, int Dout,
                                  float slope, float p, unsigned long seed, unsigned long stream_id, const float* h, const float* g_out,
                                  long out_ld, const float* g_h, float* ds, float* dx_direct, float* dW1, float* dW2, float* dbias,
                                  void* workspace, long workspace_bytes, void* stream) {
  NgArgs a;
  a.who = "sbr_ngcf_layer_bwd";
  if (int rc = ng_check(&a, u_indptr, u_indices, i_indptr, i_indices, n_users, n_items, r0, r1, Din, Dout, slope, p, seed, stream_id)) return rc;
  SBR_REQUIRE(out_ld >= Dout, "%s: out_ld=%ld below Dout=%d", a.who, out_ld, Dout);
  const long wb = 4L * Din * Dout, need = (long)ng_bwd_ws_bytes(r1 - r0, Din, Dout);
  const NgSpan spans[] = {{"x", x, 4 * a.n * Din, false}, {"W1", W1, wb, false}, {"W2", W2, wb, false}, {"h", h, 4 * a.n * Dout, false},
                          {"g_out", g_out, a.n > 0 ? 4 * ((a.n - 1) * out_ld + Dout) : 0, false}, {"g_h", g_h, 4 * a.n * Dout, false},
                          {"ds", ds, 4 * a.n * Din, true}, {"dx_direct", dx_direct, 4 * a.n * Din, true}, {"dW1", dW1, wb, true},
                          {"dW2", dW2, wb, true}, {"dbias", dbias, 4L * Dout, true}, {"workspace", workspace, need, true}};
  if (int rc = ng_disjoint(a.who, spans, 12)) return rc;
  if (r0 == r1) return SBR_OK;
  SBR_REQUIRE(u_indptr && i_indptr && x && W1 && W2 && h && g_out && ds && dx_direct && dW1 && dW2 && dbias, "%s: null operand", a.who);
  SBR_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %ld bytes, needs %ld", a.who, workspace_bytes, need);
  bool vec;
  int gshift, per_lane;
  ng_group(x, Din, &vec, &gshift, &per_lane);
  hipStream_t st = (hipStream_t)stream;
  const int nb = ng_splits(r1 - r0, Din, Dout);
  float* part = (float*)workspace;
  int rc = SBR_OK;
#define NG_ARGS a, x, W1, W2, h, g_out, out_ld, g_h, ds, dx_direct, part, nb, gshift, st
#define NG_GO2(V, C, NPT) (Din <= T64_T ? ng_bwd_launch<V, C, NPT, 1>(NG_ARGS) : ng_bwd_launch<V, C, NPT, 2>(NG_ARGS))
#define NG_GO(V, C) (Dout <= T64_T ? NG_GO2(V, C, 1) : NG_GO2(V, C, 2))
  if (vec) rc = NG_GO(4, 1);
  else if (per_lane <= 1) rc = NG_GO(1, 1);
  else rc = NG_GO(1, 2);
#undef NG_GO
#undef NG_GO2
#undef NG_ARGS
  if (rc) return rc;
  const long DD = (long)Din * Dout;
  t64_fold_kernel<<<sbr_cdiv(DD, 256), 256, 0, st>>>(part, nullptr, nb, Din, Dout, NgFoldEpi{}, dW1);
  t64_fold_kernel<<<sbr_cdiv(DD, 256), 256, 0, st>>>(part + nb * DD, nullptr, nb, Din, Dout, NgFoldEpi{}, dW2);
  t64_fold_kernel<<<sbr_cdiv(Dout, 256), 256, 0, st>>>(part + 2 * nb * DD, nullptr, nb, 1, Dout, NgFoldEpi{}, dbias);
  SBR_CHECK_LAUNCH(a.who);
  return SBR_OK;
}
