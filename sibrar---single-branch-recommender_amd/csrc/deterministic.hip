// Deterministic mode: the process-wide switch, the counter of arrival-order launches, and the two families of fixed-order kernels
// the other files route their accumulations through while the switch is on (det.h; reference call site utilities/utils.py:22-27:
// seeds + cudnn.deterministic — "same seed, same model").
//
//   segmented row accumulation   dW[rows[j], :] += dOut[ii(j), :]: the grouping by destination row is built on the device (hash of the
//                                distinct rows, counts, segment placement — integer atomics only, none of which decides a value),
//                                every segment is brought into ascending source position, and ONE wave owns a destination row: it adds
//                                the segment's rows in that order and writes the row with plain vector stores.
//   fixed-slot column reduction  every workgroup of a column reduction stores its partial sums in the slot of its own blockIdx
//                                (colred.h: sbr_colred_publish with `slots`), sbr_det_fold_slots adds the slots in a fixed pattern.
#include "det.h"
#include <atomic>
#include <mutex>

static std::atomic<int> g_det{0};
static std::atomic<long> g_arrival_launches{0};

bool sbr_det_on() { return g_det.load(std::memory_order_relaxed) != 0; }
void sbr_note_arrival_order() { g_arrival_launches.fetch_add(1, std::memory_order_relaxed); }

extern "C" int sbr_set_deterministic(int on) {
  g_det.store(on ? 1 : 0, std::memory_order_relaxed);
  return SBR_OK;
}
extern "C" int sbr_get_deterministic(void) { return g_det.load(std::memory_order_relaxed); }
extern "C" long sbr_nondeterministic_launches(void) { return g_arrival_launches.load(std::memory_order_relaxed); }
extern "C" int sbr_reset_nondeterministic_launches(void) {
  g_arrival_launches.store(0, std::memory_order_relaxed);
  return SBR_OK;
}

// ---- scratch --------------------------------------------------------------------------------------------------------------
#define SBR_DET_MAX_DEV 64
struct DetScratch { void* p; size_t bytes; };
static DetScratch g_scratch[SBR_DET_MAX_DEV][3];
static std::mutex g_scratch_mu;

void* sbr_det_scratch(int purpose, size_t bytes, hipStream_t s, const char* entry) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SBR_DET_MAX_DEV || purpose < 0 || purpose > 2) {
    sbr_set_error("%s: no device for the deterministic scratch", entry);
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  DetScratch& g = g_scratch[dev][purpose];
  if (g.p && g.bytes >= bytes) return g.p;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    sbr_set_error("%s: the deterministic scratch must grow to %zu bytes, which a capturing stream cannot allocate (run one plain step first)",
                  entry, bytes);
    return nullptr;
  }
  size_t want = bytes > 2 * g.bytes ? bytes : 2 * g.bytes;
  want = (want + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  void* p = nullptr;
  if (hipMalloc(&p, want) != hipSuccess) {
    (void)hipGetLastError();
    sbr_set_error("%s: cannot allocate %zu bytes of deterministic scratch", entry, want);
    return nullptr;
  }
  g.p = p;                       // the outgrown block is retired, not freed: captured steps and queued launches hold its address
  g.bytes = want;
  return p;
}

// ---- fixed-slot column reduction: slots -> replica 1 of the workspace ---------------------------------------------------------------
// block = 16 columns x 16 slot lanes: lane q adds slots q, q + 16, ... (ascending), the 16 lane sums are added in lane order
__global__ __launch_bounds__(256) void det_fold_slots_kernel(const double* __restrict__ slots, int nslots, int KD, double* __restrict__ ws) {
  __shared__ double sm[16][17];
  const int cl = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;
  double s = 0.0;
  if (col < KD)
    for (int r = q; r < nslots; r += 16) s += slots[(long)r * KD + col];
  sm[q][cl] = s;
  __syncthreads();
  if (q == 0 && col < KD) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sm[k][cl];
    ws[KD + col] = t;
  }
}

int sbr_det_fold_slots(const double* slots, int nslots, int KD, double* ws, hipStream_t s, const char* entry) {
  det_fold_slots_kernel<<<sbr_cdiv(KD, 16), 256, 0, s>>>(slots, nslots, KD, ws);
  SBR_CHECK_LAUNCH(entry);
  return SBR_OK;
}

// thread i adds partials i, i + 256, ...; the 256 thread sums go through the wave butterfly and the four wave sums are added in order
__global__ __launch_bounds__(256) void det_sum_partials_kernel(const double* __restrict__ partials, int n, double* __restrict__ out) {
  __shared__ double sm[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
  s = sbr_wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

int sbr_det_sum_partials(const double* partials, int n, double* out, hipStream_t s, const char* entry) {
  det_sum_partials_kernel<<<1, 256, 0, s>>>(partials, n, out);
  SBR_CHECK_LAUNCH(entry);
  return SBR_OK;
}

// ---- segmented row accumulation -------------------------------------------------------------------------------------------
struct DetScatterWs {
  int* keys;      // [H] destination row of a hash entry, -1: free
  int* cnt;       // [H] source rows of the entry's segment
  int* start;     // [H] where the segment begins in `placed`
  int* cursor;    // [H] placement cursor (decides positions inside `placed`, which are re-ordered before they decide anything)
  int* seglist;   // [n] hash entries in use
  int* slotof;    // [n] hash entry of source position j, -1: a zero row (skipped) or a negative destination
  int* placed;    // [n] source positions, grouped by segment
  int* ctr;       // [0] rows placed, [1] segments
  int H, logH;
};

__global__ void det_scatter_init_kernel(DetScatterWs w) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < w.H) { w.keys[e] = -1; w.cnt[e] = 0; w.cursor[e] = 0; }
  if (e == 0) { w.ctr[0] = 0; w.ctr[1] = 0; }
}

// one wave per source position: is the gradient row zero (the ~770 padded slots of a graph-mode step name ONE table row with a zero
// gradient row: engine._EntityRun.plan — left out like the atomic kernel leaves them out), else claim / find the hash entry of its
// destination row and count
__global__ __launch_bounds__(256) void det_scatter_mark_kernel(const float* __restrict__ dOut, long ldo, const int* __restrict__ in_idx,
                                                               const int* __restrict__ rows, long n, int D, DetScatterWs w) {
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  for (long j = wid; j < n; j += nw) {
    const long src = in_idx ? (long)in_idx[j] : j;
    bool nz = false;
    for (int c = lane; c < D; c += 64) nz |= dOut[src * ldo + c] != 0.f;
    const bool any = __ballot(nz) != 0;
    if (lane == 0) {
      const int r = rows[j];
      int slot = -1;
      if (any && r >= 0) {
        unsigned h = ((unsigned)r * 2654435761u) >> (32 - w.logH);
        for (;;) {                                      // at most n distinct rows in H >= 2 n entries: a free entry exists
          const int old = atomicCAS(&w.keys[h], -1, r);
          if (old == -1 || old == r) break;
          h = (h + 1) & (unsigned)(w.H - 1);
        }
        atomicAdd(&w.cnt[h], 1);
        slot = (int)h;
      }
      w.slotof[j] = slot;
    }
  }
}

__global__ void det_scatter_segments_kernel(DetScatterWs w) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= w.H || w.keys[e] == -1) return;
  w.start[e] = atomicAdd(&w.ctr[0], w.cnt[e]);
  w.seglist[atomicAdd(&w.ctr[1], 1)] = e;
}

__global__ void det_scatter_place_kernel(long n, DetScatterWs w) {
  const long j = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int s = w.slotof[j];
  if (s >= 0) w.placed[w.start[s] + atomicAdd(&w.cursor[s], 1)] = (int)j;
}

#define DET_WAVE_SYNC()                                     \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
    __builtin_amdgcn_wave_barrier();                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
  } while (0)

// acc += the rows named by list[0 .. cnt) (ascending source positions, in LDS), in list order; four rows in flight
template <int NC>
__device__ __forceinline__ void det_add_list(const float* __restrict__ dOut, long ldo, const int* __restrict__ in_idx, const int* list,
                                             int cnt, int D, int lane, float (&acc)[NC]) {
  for (int t = 0; t < cnt; t += 4) {
    float v[4][NC];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = list[t + q < cnt ? t + q : cnt - 1];
      const long src = in_idx ? (long)in_idx[p] : (long)p;
#pragma unroll
      for (int i = 0; i < NC; ++i) v[q][i] = (lane + 64 * i < D) ? dOut[src * ldo + lane + 64 * i] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (t + q < cnt) {
#pragma unroll
        for (int i = 0; i < NC; ++i) acc[i] += v[q][i];
      }
  }
}

// one wave per segment. Up to 64 rows: the wave ranks the segment's source positions (a position's rank = how many of the others are
// smaller) and adds in rank order. Longer segments (one popular row; a test that sends every row to one destination) ignore the
// placement and walk ALL source positions in order, 64 at a time, taking those of the segment: n / 64 wave steps per long segment,
// and there are at most n / 64 of them.
template <int NC>
__global__ __launch_bounds__(256) void det_scatter_add_kernel(const float* __restrict__ dOut, long ldo, const int* __restrict__ in_idx,
                                                              float* __restrict__ dW, long ldw, long n, int D, DetScatterWs w) {
  __shared__ int sm[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nseg = w.ctr[1];
  int* list = sm[wave];
  for (int sidx = blockIdx.x * 4 + wave; sidx < nseg; sidx += gridDim.x * 4) {
    const int h = w.seglist[sidx];
    const int L = w.cnt[h], st = w.start[h];
    const long r = w.keys[h];
    float acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.f;
    if (L <= 64) {
      const int pos = lane < L ? w.placed[st + lane] : 0x7fffffff;
      int rank = 0;
      for (int k = 0; k < L; ++k) rank += __shfl(pos, k, 64) < pos;
      if (lane < L) list[rank] = pos;
      DET_WAVE_SYNC();
      det_add_list<NC>(dOut, ldo, in_idx, list, L, D, lane, acc);
      DET_WAVE_SYNC();
    } else {
      for (long base = 0; base < n; base += 64) {
        const long j = base + lane;
        const bool mine = j < n && w.slotof[j] == h;
        const unsigned long long mask = __ballot(mine);
        if (mask == 0) continue;                                    // wave-uniform
        if (mine) list[__popcll(mask & ((1ull << lane) - 1ull))] = (int)j;
        DET_WAVE_SYNC();
        det_add_list<NC>(dOut, ldo, in_idx, list, __popcll(mask), D, lane, acc);
        DET_WAVE_SYNC();
      }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i)
      if (lane + 64 * i < D) dW[r * ldw + lane + 64 * i] += acc[i];
  }
}

int sbr_det_scatter_add_rows(const float* dOut, long ldo, const int* in_idx, const int* rows, float* dW, long ldw, long n, int D,
                             hipStream_t s, const char* entry) {
  if (n == 0) return SBR_OK;
  SBR_REQUIRE(D >= 1 && D <= 512, "%s: no deterministic form for rows of %d floats (1 .. 512)", entry, D);
  SBR_REQUIRE(n < (1L << 28), "%s: no deterministic form for %ld rows", entry, n);
  DetScatterWs w;
  w.logH = 6;
  while ((1L << w.logH) < 2 * n) ++w.logH;
  w.H = 1 << w.logH;
  const size_t ints = 4 * (size_t)w.H + 3 * (size_t)n + 16;
  int* base = (int*)sbr_det_scratch(SBR_SCRATCH_SCATTER, ints * sizeof(int), s, entry);
  if (!base) return SBR_ERR_HIP;
  w.keys = base;
  w.cnt = w.keys + w.H;
  w.start = w.cnt + w.H;
  w.cursor = w.start + w.H;
  w.seglist = w.cursor + w.H;
  w.slotof = w.seglist + n;
  w.placed = w.slotof + n;
  w.ctr = w.placed + n;
  det_scatter_init_kernel<<<sbr_cdiv(w.H, 256), 256, 0, s>>>(w);
  int mb = sbr_cdiv(n, 4);
  if (mb > 4096) mb = 4096;
  det_scatter_mark_kernel<<<mb, 256, 0, s>>>(dOut, ldo, in_idx, rows, n, D, w);
  det_scatter_segments_kernel<<<sbr_cdiv(w.H, 256), 256, 0, s>>>(w);
  det_scatter_place_kernel<<<sbr_cdiv(n, 256), 256, 0, s>>>(n, w);
  int ab = sbr_cdiv(n, 4);
  if (ab > 2048) ab = 2048;
  const int nc = sbr_cdiv(D, 64);
  if (nc == 1) det_scatter_add_kernel<1><<<ab, 256, 0, s>>>(dOut, ldo, in_idx, dW, ldw, n, D, w);
  else if (nc == 2) det_scatter_add_kernel<2><<<ab, 256, 0, s>>>(dOut, ldo, in_idx, dW, ldw, n, D, w);
  else if (nc <= 4) det_scatter_add_kernel<4><<<ab, 256, 0, s>>>(dOut, ldo, in_idx, dW, ldw, n, D, w);
  else det_scatter_add_kernel<8><<<ab, 256, 0, s>>>(dOut, ldo, in_idx, dW, ldw, n, D, w);
  SBR_CHECK_LAUNCH(entry);
  return SBR_OK;
}

// the fixed-order form as an entry point of its own (what sbr_scatter_add_rows runs while the mode is on): callable in either mode
extern "C" int sbr_scatter_add_rows_det(const float* dOut, long ldo, const int* in_idx, const int* rows, float* dW, long ldw, long n,
                                        int D, void* stream) {
  if (n == 0) return SBR_OK;
  SBR_REQUIRE(dOut && rows && dW, "sbr_scatter_add_rows_det: null operand");
  return sbr_det_scatter_add_rows(dOut, ldo, in_idx, rows, dW, ldw, n, D, (hipStream_t)stream, "sbr_scatter_add_rows_det");
}
