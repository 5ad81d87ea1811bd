// Exceedance objects (include/downgan_hip.h "Exceedance objects"): the connected components of the masks y > thr[j][k] of one or
// two series of H x W fields read through the EOF descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16), one 12-column int64
// record per object: plane, root (smallest pixel index), area, overlap with the other side's mask, fixed-point mass and first
// moments, peak, bounding box.
//   obj_init_kernel<T, MODE>    one wave per row (t, h) of one side: 64 pixels per step, the output values y of hist_common.h, the
//                               masks of all (j, k) as wave ballots; a set pixel's label = the index of the first pixel of its
//                               horizontal run (from the ballot, wave-uniform carry across the chunks), a clear pixel's = -1
//   obj_merge_kernel            one thread per pixel and plane: joins the pixel's run with the set neighbours of the row above by
//                               lock-free union-find (find both roots, atomicMin the smaller into the larger root's label,
//                               continue from the value returned); a pixel whose left neighbour already made the same join skips it
//   obj_flatten_kernel          label[p] = find(p): links only point to smaller member indices, so the root is the smallest index
//   obj_slots_kernel            every root draws a record slot (one counter atomic and one per_plane atomic per wave), writes the
//                               initial record when the slot is below capacity and stores the slot id in the second int32 plane
//   obj_stats_kernel<T, MODE>   one wave per row again: q of every pixel, per (j, k) the runs of equal root among the 64 lanes
//                               (ballots), their sums from wave prefix sums, one set of 64-bit integer atomics per run
// Progress: no lane, wave or workgroup waits for a value another one writes; find and union walk strictly decreasing indices under
// a hard cap of P steps, at which they set the error word of the workspace and leave (dg_objects then returns DG_ERR_LAUNCH).
// Everything is integer after the compare and the rounding: exact, independent of arrival order; the row order alone is not fixed.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int OBJ_THREADS = 256;
constexpr int OBJ_WAVES = OBJ_THREADS / 64;
constexpr int OBJ_GRID_T = 4096;                      // fields across gridDim.y at most; the row kernels stride over the rest
constexpr int OBJ_GRID_PLANES = 16384;                // planes across gridDim.y at most; the plane kernels stride over the rest
constexpr int MAXO = DG_HIST_MAX_OUT, MAXK = DG_OBJ_MAX_THR, COLS = DG_OBJ_COLS;
constexpr size_t OBJ_HEADER = 256;                    // bytes in front of the planes: the error word
constexpr long long QMAX = (1 << 24) - 1;

typedef unsigned long long u64;

// Definition, shared by the kernels and the host reference: one correctly rounded fp32 multiply, then round to nearest even.
__host__ __device__ inline long long obj_q(float y, float inv_quantum) {
#pragma clang fp contract(off)
  const float t = y * inv_quantum;
  if (t >= 16777215.f) return QMAX;
  if (!(t > 0.f)) return 0;                           // negative, zero (and NaN, which no mask holds)
  return (long long)__builtin_rintf(t);
}

struct ObjRowArgs {
  HistSeries x;
  HistXform xf;
  int H, W, T, nout, nthr, side, paired;
  float inv_quantum;
  float thr[MAXO][MAXK];
  int* labels;                // plane ((t * 2 + side) * nout + j) * nthr + k, H * W entries each
  const int* slots;           // the same planes: the record slot of every root pixel
  u64* table;
  long long capacity;
};

template <typename T, int MODE>
__global__ __launch_bounds__(OBJ_THREADS) void obj_init_kernel(ObjRowArgs g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.x * OBJ_WAVES + wave;
  if (h >= g.H) return;                                              // wave-uniform
  const long long P = (long long)g.H * g.W;
  const T* base = reinterpret_cast<const T*>(g.x.base);
  const u64 below = (1ull << lane) - 1ull;                           // lanes 0 .. lane - 1
  const int row = h * g.W;
  for (int t = blockIdx.y; t < g.T; t += gridDim.y) {
    int carry[MAXO][MAXK];                                           // the start of the run that reaches the chunk's left edge, or -1
#pragma unroll
    for (int j = 0; j < MAXO; ++j)
#pragma unroll
      for (int k = 0; k < MAXK; ++k) carry[j][k] = -1;
    int* field = g.labels + ((long long)t * 2 + g.side) * g.nout * g.nthr * P + row;
    for (int w0 = 0; w0 < g.W; w0 += 64) {
      const int w = w0 + lane;
      const bool in = w < g.W;
      const long long p = (long long)row + (in ? w : g.W - 1);       // lanes beyond the row read its last pixel, unused
      float y[MAXO];
      hist_pixel_values<T, MODE>(g.xf, base + t * g.x.ld_t + p * g.x.ld_p, g.x.ld_c, y);
#pragma unroll
      for (int j = 0; j < MAXO; ++j) {
        if (j < g.nout) {
#pragma unroll
          for (int k = 0; k < MAXK; ++k) {
            if (k < g.nthr) {
              const u64 m = __ballot(in && y[j] > g.thr[j][k]);
              const int edge = carry[j][k] >= 0 ? carry[j][k] : row + w0;   // the label of a run that starts at lane 0
              const u64 zeros = ~m & below;
              const int start = zeros ? row + w0 + 64 - __clzll((long long)zeros) : edge;
              if (in) field[(long long)(j * g.nthr + k) * P + w] = (m >> lane) & 1ull ? start : -1;
              const u64 nz = ~m;
              carry[j][k] = m >> 63 ? (nz ? row + w0 + 64 - __clzll((long long)nz) : edge) : -1;
            }
          }
        }
      }
    }
  }
}

__device__ __forceinline__ int obj_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see: x -> label[x] while that is smaller.  Strictly decreasing; at most `cap` steps.
__device__ __forceinline__ int obj_find(const int* L, int x, int cap, int* err) {
  for (int s = 0; s < cap; ++s) {
    const int y = obj_load(L + x);
    if (y >= x || y < 0) return x;
    x = y;
  }
  *err = 1;
  return x;
}

// join the components of a and b: the larger root's label takes the smaller root.  When the atomic finds that the larger one was
// no root any more, the value it returns (its parent, smaller) still has to be joined with the other root: continue from there.
// a + b decreases strictly in every round.
__device__ __forceinline__ void obj_unite(int* L, int a, int b, int cap, int* err) {
  a = obj_find(L, a, cap, err);
  b = obj_find(L, b, cap, err);
  for (int s = 0; a != b; ++s) {
    if (s >= cap) { *err = 1; return; }
    if (a < b) { const int x = a; a = b; b = x; }                    // a > b
    const int old = atomicMin(L + a, b);
    if (old == a) return;                                            // a was a root and now points to b
    a = obj_find(L, old, cap, err);                                  // old < a
    b = obj_find(L, b, cap, err);
  }
}

__global__ __launch_bounds__(OBJ_THREADS) void obj_merge_kernel(int* labels, long long nplanes, int H, int W, int conn8, int* err) {
  const int P = H * W;
  const int p = blockIdx.x * OBJ_THREADS + threadIdx.x;
  if (p >= P || p < W) return;                                       // row 0 has nothing above it
  const int w = p % W;
  for (long long plane = blockIdx.y; plane < nplanes; plane += gridDim.y) {
    int* L = labels + plane * P;
    if (L[p] < 0) continue;                                          // the sign of a label never changes: a plain load
    const bool n = L[p - W] >= 0;
    const bool left = w > 0 && L[p - 1] >= 0;
    const bool nw = w > 0 && L[p - W - 1] >= 0;
    if (n) {
      if (!(left && nw)) obj_unite(L, p, p - W, P, err);             // else the left neighbour joined the same two runs
    } else if (conn8) {
      if (nw && !left) obj_unite(L, p, p - W - 1, P, err);
      if (w + 1 < W && L[p - W + 1] >= 0) obj_unite(L, p, p - W + 1, P, err);
    }
  }
}

__global__ __launch_bounds__(OBJ_THREADS) void obj_flatten_kernel(int* labels, long long nplanes, int P, int* err) {
  const int p = blockIdx.x * OBJ_THREADS + threadIdx.x;
  if (p >= P) return;
  for (long long plane = blockIdx.y; plane < nplanes; plane += gridDim.y) {
    int* L = labels + plane * P;
    if (L[p] < 0) continue;
    const int r = obj_find(L, p, P, err);
    __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // a root or the old parent: both valid to a reader
  }
}

__global__ __launch_bounds__(OBJ_THREADS) void obj_slots_kernel(const int* labels, int* slots, long long nplanes, int P, int W,
                                                                u64* table, long long capacity, u64* count, u64* per_plane) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * OBJ_THREADS + threadIdx.x;              // a wave: 64 consecutive pixels of one plane
  for (long long plane = blockIdx.y; plane < nplanes; plane += gridDim.y) {   // workgroup-uniform
    const bool root = p < P && labels[plane * P + p] == p;
    const u64 m = __ballot(root);
    if (m == 0ull) continue;                                         // wave-uniform
    const int n = __popcll(m);
    u64 first = 0ull;
    if (lane == 0) {
      first = atomicAdd(count, (u64)n);
      atomicAdd(per_plane + plane, (u64)n);
    }
    const unsigned lo = (unsigned)__shfl((int)(unsigned)first, 0, 64), hi = (unsigned)__shfl((int)(unsigned)(first >> 32), 0, 64);
    if (root) {
      const long long slot = (long long)(((u64)hi << 32) | lo) + __popcll(m & ((1ull << lane) - 1ull));
      slots[plane * P + p] = (int)slot;                              // below 2^31: dg_objects_ws_bytes admits no larger call
      if (slot < capacity) {
        u64* r = table + slot * COLS;
        const u64 h = (u64)(p / W), w = (u64)(p % W);
        r[0] = (u64)plane; r[1] = (u64)p;
        r[2] = r[3] = r[4] = r[5] = r[6] = r[7] = 0ull;
        r[8] = h; r[9] = h; r[10] = w; r[11] = w;
      }
    }
  }
}

template <typename T, int MODE>
__global__ __launch_bounds__(OBJ_THREADS) void obj_stats_kernel(ObjRowArgs g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.x * OBJ_WAVES + wave;
  if (h >= g.H) return;                                              // wave-uniform
  const long long P = (long long)g.H * g.W;
  const T* base = reinterpret_cast<const T*>(g.x.base);
  const u64 upto = ~0ull >> (63 - lane);                             // lanes 0 .. lane
  const int row = h * g.W;
  for (int t = blockIdx.y; t < g.T; t += gridDim.y) {
    const long long njk = (long long)g.nout * g.nthr;
    const int* mine = g.labels + ((long long)t * 2 + g.side) * njk * P + row;
    const int* other = g.labels + ((long long)t * 2 + (1 - g.side)) * njk * P + row;
    const int* slot0 = g.slots + ((long long)t * 2 + g.side) * njk * P;
    for (int w0 = 0; w0 < g.W; w0 += 64) {
      const int w = w0 + lane;
      const bool in = w < g.W;
      const long long p = (long long)row + (in ? w : g.W - 1);
      float y[MAXO];
      hist_pixel_values<T, MODE>(g.xf, base + t * g.x.ld_t + p * g.x.ld_p, g.x.ld_c, y);
#pragma unroll
      for (int j = 0; j < MAXO; ++j) {
        if (j < g.nout) {
          // inclusive wave prefix sums of q (< 2^30) and q * lane (< 2^36), shared by the thresholds of channel j
          const unsigned q = in ? (unsigned)obj_q(y[j], g.inv_quantum) : 0u;
          unsigned pq = q;
          u64 pl = (u64)q * (unsigned)lane;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const unsigned a = (unsigned)__shfl_up((int)pq, o, 64);
            const unsigned lo = (unsigned)__shfl_up((int)(unsigned)pl, o, 64), hi = (unsigned)__shfl_up((int)(unsigned)(pl >> 32), o, 64);
            if (lane >= o) {
              pq += a;
              pl += ((u64)hi << 32) | lo;
            }
          }
          for (int k = 0; k < g.nthr; ++k) {
            const long long jk = (long long)j * g.nthr + k;
            const int r = in ? mine[jk * P + w] : -1;                // the root, -1 for a clear pixel
            const u64 set = __ballot(r >= 0);
            if (set == 0ull) continue;                               // wave-uniform
            const u64 oset = g.paired ? __ballot(in && other[jk * P + w] >= 0) : 0ull;
            const int prev = __shfl_up(r, 1, 64);
            const u64 heads = __ballot(lane == 0 || prev != r);      // the first lane of every run of equal roots
            const u64 rest = heads & ~upto;
            const int end = rest ? __ffsll((long long)rest) - 1 : 64;   // one past the last lane of this lane's run
            // the run's peak: a suffix maximum that stops at the run's end
            unsigned qm = q;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
              const unsigned a = (unsigned)__shfl_down((int)qm, o, 64);
              if (lane + o < end) qm = a > qm ? a : qm;
            }
            // the sums of the run of a head lane: prefix at its last lane minus the prefix in front of the head
            const unsigned eq = (unsigned)__shfl((int)pq, end - 1, 64);
            const unsigned elo = (unsigned)__shfl((int)(unsigned)pl, end - 1, 64), ehi = (unsigned)__shfl((int)(unsigned)(pl >> 32), end - 1, 64);
            if (r >= 0 && ((heads >> lane) & 1ull)) {
              const long long slot = slot0[jk * P + r];
              if (slot < g.capacity) {
                const u64 segmask = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~(upto >> 1);   // lanes lane .. end - 1
                const u64 area = (u64)(end - lane), ovl = (u64)__popcll(oset & segmask);
                const u64 mass = (u64)(eq - (pq - q));
                const u64 ql = (((u64)ehi << 32) | elo) - (pl - (u64)q * (unsigned)lane);
                u64* rec = g.table + slot * COLS;
                const int rh = r / g.W, rw = r % g.W;
                atomicAdd(rec + 2, area);
                if (ovl) atomicAdd(rec + 3, ovl);
                if (mass) {
                  atomicAdd(rec + 4, mass);
                  if (h) atomicAdd(rec + 5, mass * (u64)h);
                  const u64 qw = mass * (u64)w0 + ql;
                  if (qw) atomicAdd(rec + 6, qw);
                  atomicMax(rec + 7, (u64)qm);
                }
                if (h > rh) atomicMax(rec + 9, (u64)h);              // h0 = the root's row, written with the record
                if (w < rw) atomicMin(rec + 10, (u64)w);
                if (w0 + end - 1 > rw) atomicMax(rec + 11, (u64)(w0 + end - 1));
              }
            }
          }
        }
      }
    }
  }
}

bool spec_ok(const dg_objects_spec* s, int C) {
  if (!s || s->nthr < 1 || s->nthr > MAXK || (s->connectivity != 4 && s->connectivity != 8)) return false;
  if (!hist_finite(s->inv_quantum) || !(s->inv_quantum > 0.f)) return false;
  return hist_xform_ok(s, C) && hist_thr_ok(s->thr, hist_nout(s, C), s->nthr);
}

bool grid_ok(int H, int W) { return H >= 1 && W >= 1 && H <= DG_OBJ_MAX_SIDE && W <= DG_OBJ_MAX_SIDE; }

long long planes_of(const dg_eof_fields* a, const dg_objects_spec* s) {
  return (long long)a->T * 2 * hist_nout(s, a->C) * s->nthr;
}

bool call_ok(const dg_eof_fields* a, int H, int W, const dg_objects_spec* s) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C) || !grid_ok(H, W) || (long long)H * W != a->P) return false;
  return planes_of(a, s) * ((a->P + 1) / 2) < (1LL << 31);           // every slot id fits an int32
}

template <bool STATS>
void rows_of(const dg_eof_fields* x, int side, ObjRowArgs g, dim3 grid, hipStream_t st) {
  g.x = hist_series(x); g.side = side;
  hist_dispatch<false>(x->dtype, hist_mode(x), [&](auto t, auto m) {
    if (STATS) hipLaunchKernelGGL((obj_stats_kernel<decltype(t), decltype(m)::value>), grid, dim3(OBJ_THREADS), 0, st, g);
    else hipLaunchKernelGGL((obj_init_kernel<decltype(t), decltype(m)::value>), grid, dim3(OBJ_THREADS), 0, st, g);
  });
}

struct HostRec { int64_t v[COLS]; };

}  // namespace

extern "C" size_t dg_objects_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_objects_spec* s) {
  if (!call_ok(a, H, W, s)) return 0;
  return OBJ_HEADER + (size_t)planes_of(a, s) * (size_t)a->P * 2 * sizeof(int);
}

extern "C" int dg_objects_host(const dg_objects_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* table,
                               int64_t capacity, int64_t* count, int64_t* per_plane) {
  if (!spec_ok(s, C) || !a || !count || !per_plane || !grid_ok(H, W) || capacity < 0 || (capacity > 0 && !table)) return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C), conn8 = s->connectivity == 8;
  const size_t P = (size_t)H * W;
  const float* x[2] = {a, b};
  std::vector<float> y[2];
  std::vector<unsigned char> mask[2], seen;
  std::vector<int> stack;
  int64_t total = 0;
  for (int i = 0; i < 2 * nout * s->nthr; ++i) per_plane[i] = 0;
  for (int side = 0; side < (b ? 2 : 1); ++side) {
    for (int j = 0; j < nout; ++j) {
      for (int e = 0; e < 2; ++e) {                                  // the values of channel j of both sides
        if (!x[e]) continue;
        y[e].resize(P);
        for (size_t p = 0; p < P; ++p) y[e][p] = hist_host_value(s, x[e], C, P, p, j);
      }
      for (int k = 0; k < s->nthr; ++k) {
        for (int e = 0; e < 2; ++e) {
          mask[e].assign(P, 0);
          if (x[e])
            for (size_t p = 0; p < P; ++p) mask[e][p] = y[e][p] > s->thr[j][k] ? 1 : 0;
        }
        const std::vector<unsigned char>& M = mask[side];
        const std::vector<unsigned char>& O = mask[1 - side];
        const int64_t plane = ((int64_t)side * nout + j) * s->nthr + k;
        seen.assign(P, 0);
        for (size_t p0 = 0; p0 < P; ++p0) {                          // in index order: the first pixel met is the root
          if (!M[p0] || seen[p0]) continue;
          HostRec r;
          r.v[0] = plane; r.v[1] = (int64_t)p0;
          for (int c = 2; c < 8; ++c) r.v[c] = 0;
          r.v[8] = r.v[9] = (int64_t)(p0 / W);
          r.v[10] = r.v[11] = (int64_t)(p0 % W);
          seen[p0] = 1;
          stack.clear();
          stack.push_back((int)p0);
          while (!stack.empty()) {
            const int p = stack.back();
            stack.pop_back();
            const int h = p / W, w = p % W;
            const int64_t q = obj_q(y[side][p], s->inv_quantum);
            r.v[2] += 1; r.v[3] += O[p]; r.v[4] += q; r.v[5] += q * h; r.v[6] += q * w;
            r.v[7] = std::max(r.v[7], q);
            r.v[8] = std::min<int64_t>(r.v[8], h); r.v[9] = std::max<int64_t>(r.v[9], h);
            r.v[10] = std::min<int64_t>(r.v[10], w); r.v[11] = std::max<int64_t>(r.v[11], w);
            for (int dh = -1; dh <= 1; ++dh) {
              for (int dw = -1; dw <= 1; ++dw) {
                if ((dh == 0 && dw == 0) || (!conn8 && dh != 0 && dw != 0)) continue;
                const int hh = h + dh, ww = w + dw;
                if (hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
                const size_t n = (size_t)hh * W + ww;
                if (M[n] && !seen[n]) {
                  seen[n] = 1;
                  stack.push_back((int)n);
                }
              }
            }
          }
          if (total < capacity) std::copy(r.v, r.v + COLS, table + total * COLS);
          ++total;
          ++per_plane[plane];
        }
      }
    }
  }
  *count = total;
  return DG_OK;
}

extern "C" int dg_objects(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_objects_spec* s, void* ws,
                          int64_t* table, int64_t capacity, int64_t* count, int64_t* per_plane, void* stream) {
  if (!call_ok(a, H, W, s) || !ws || !count || !per_plane || capacity < 0 || (capacity > 0 && !table)) return DG_ERR_BAD_SHAPE;
  if (b && (!hist_fields_ok(b) || b->T != a->T || b->C != a->C || b->P != a->P)) return DG_ERR_BAD_SHAPE;
  if ((a->dtype != DG_F32 && a->dtype != DG_BF16) || (b && b->dtype != DG_F32 && b->dtype != DG_BF16)) return DG_ERR_BAD_DTYPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long long nplanes = planes_of(a, s), P = a->P;
  const int nout = hist_nout(s, a->C);
  int* err = reinterpret_cast<int*>(ws);
  int* labels = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + OBJ_HEADER);
  int* slots = labels + nplanes * P;
  if (hipMemsetAsync(ws, 0, OBJ_HEADER, st) != hipSuccess) return DG_ERR_LAUNCH;
  if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) return DG_ERR_LAUNCH;
  if (hipMemsetAsync(per_plane, 0, (size_t)nplanes * sizeof(int64_t), st) != hipSuccess) return DG_ERR_LAUNCH;
  // the side-1 planes of a one-series call hold no object: all labels -1 (every byte 0xff)
  if (!b && hipMemsetAsync(labels, 0xff, (size_t)nplanes * P * sizeof(int), st) != hipSuccess) return DG_ERR_LAUNCH;

  ObjRowArgs g;
  g.xf = hist_xform(s, a->C);
  g.H = H; g.W = W; g.T = a->T; g.nout = nout; g.nthr = s->nthr; g.paired = b ? 1 : 0;
  g.inv_quantum = s->inv_quantum;
  hist_thr_pad(s->thr, nout, s->nthr, g.thr);
  g.labels = labels; g.slots = slots; g.table = reinterpret_cast<u64*>(table); g.capacity = capacity;
  const unsigned gt = (unsigned)(a->T < OBJ_GRID_T ? a->T : OBJ_GRID_T);
  const dim3 rgrid((unsigned)((H + OBJ_WAVES - 1) / OBJ_WAVES), gt);
  rows_of<false>(a, 0, g, rgrid, st);
  if (b) rows_of<false>(b, 1, g, rgrid, st);

  const dim3 pgrid((unsigned)((P + OBJ_THREADS - 1) / OBJ_THREADS), (unsigned)(nplanes < OBJ_GRID_PLANES ? nplanes : OBJ_GRID_PLANES));
  if (H > 1)
    hipLaunchKernelGGL(obj_merge_kernel, pgrid, dim3(OBJ_THREADS), 0, st, labels, nplanes, H, W, s->connectivity == 8 ? 1 : 0, err);
  hipLaunchKernelGGL(obj_flatten_kernel, pgrid, dim3(OBJ_THREADS), 0, st, labels, nplanes, (int)P, err);
  hipLaunchKernelGGL(obj_slots_kernel, pgrid, dim3(OBJ_THREADS), 0, st, (const int*)labels, slots, nplanes, (int)P, W,
                     reinterpret_cast<u64*>(table), (long long)capacity, reinterpret_cast<u64*>(count), reinterpret_cast<u64*>(per_plane));
  rows_of<true>(a, 0, g, rgrid, st);
  if (b) rows_of<true>(b, 1, g, rgrid, st);
  if (dg_check_launch() != DG_OK) return DG_ERR_LAUNCH;
  int failed = 0;                                                    // the step cap of find / union was reached: no table
  if (hipMemcpyAsync(&failed, err, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return DG_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return DG_ERR_LAUNCH;
  return failed ? DG_ERR_LAUNCH : DG_OK;
}
