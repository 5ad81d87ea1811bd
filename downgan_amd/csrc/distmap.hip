// Distance maps (include/downgan_hip.h "Distance maps"): the exact squared Euclidean distance transform of the masks y > thr[j][k]
// of one or two series of H x W fields read through the EOF descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16), and from it
// one 11-column int64 record per field pair and (j, k) (mean error distance, Hausdorff, Baddeley sums) and the ring counts.
//   dist_down_kernel<T, MODE>   one thread per column w of one (t, side): walks down the column once, the output values y of
//                               hist_common.h, for every (j, k) the last set row; writes g = the distance to the nearest set pixel
//                               above as uint16 (0xFFFF: none).  Coalesced along w; the loads of four rows are issued together
//   dist_up_kernel              one thread per column of one plane: walks up, reads g back (0 = a set pixel) and lowers it to the
//                               distance to the nearest set pixel below
//   dist_rows_kernel            one workgroup per row h of (t, j, k), both sides: g^2 of the row in LDS as int32 (FAR for none);
//                               a thread owns the pixels w, w + 256, ... and scans outward, best = min(best, D^2 + g^2[w +- D]) while
//                               D^2 < best (no candidate with D^2 >= best can win: exact); a row without any finite g is a row of
//                               an empty plane (g is the distance within the whole column), so the scan is skipped; the same thread
//                               forms ring, dq and w of both sides; sums and maxima are reduced over the wave, one set of 64-bit
//                               integer atomics per wave; the ring bins go to an LDS table flushed once per workgroup
//   dist_finalize_kernel        one thread per record: columns 3 .. 8 = -1 unless both masks hold a pixel
// The workspace is the g planes alone: 2 bytes per plane pixel.  Everything is integer after the compare: exact, independent of
// arrival order.  No lane, wave or workgroup waits for a value another one writes (the kernels follow each other on the stream).
#include <float.h>
#include <math.h>

#include <vector>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int COL_THREADS = 64;
constexpr int ROW_THREADS = 256;
constexpr int DOWN_ROWS = 4, UP_ROWS = 8;             // rows whose loads a column thread issues before it uses them
constexpr int DIST_GRID_PLANES = 16384;               // planes across gridDim.y at most; the up kernel strides over the rest
constexpr int DIST_GRID_T = 4096;                     // fields across gridDim.y at most; the kernels stride over the rest
constexpr int MAXO = DG_HIST_MAX_OUT, MAXK = DG_DIST_MAX_THR, COLS = DG_DIST_COLS;
constexpr int FAR = DG_DIST_FAR;
constexpr int NONE = 0xFFFF;                          // g of a column without a set pixel
constexpr int MAXBINS = DG_DIST_MAX_RINGS + 2;

typedef unsigned long long u64;

// Definitions, shared by the kernels and the host reference: integers after a first guess that only has to be close.
// ring: the smallest r with d2 <= r * r (0 <= d2 <= FAR)
__host__ __device__ inline int dist_ring(int d2) {
  int r = (int)__builtin_sqrtf((float)d2);
  while (r * r > d2) --r;
  while ((r + 1) * (r + 1) <= d2) ++r;
  return r * r == d2 ? r : r + 1;
}
// dq: floor(sqrt(d2 * 2^20)), the distance in units of 2^-10 px (0 <= d2 <= FAR: d2 * 2^20 <= 2^50)
__host__ __device__ inline long long dist_dq(int d2) {
  const u64 n = (u64)d2 << 20;
  u64 r = (u64)__builtin_sqrt((double)n);
  while (r * r > n) --r;
  while ((r + 1) * (r + 1) <= n) ++r;
  return (long long)r;
}

struct DistColArgs {
  HistSeries x;
  HistXform xf;
  int H, W, T, nout, nthr, side;
  float thr[MAXO][MAXK];
  unsigned short* g;          // plane ((t * 2 + side) * nout + j) * nthr + k, H * W entries each
};

template <typename T, int MODE>
__global__ __launch_bounds__(COL_THREADS) void dist_down_kernel(DistColArgs g) {
  const int w = blockIdx.x * COL_THREADS + threadIdx.x;
  if (w >= g.W) return;
  const long long P = (long long)g.H * g.W;
  const int njk = g.nout * g.nthr;
  const T* base = reinterpret_cast<const T*>(g.x.base);
  for (int t = blockIdx.y; t < g.T; t += gridDim.y) {
    unsigned short* G = g.g + ((long long)t * 2 + g.side) * njk * P + w;
    int last[MAXO][MAXK];                                            // the last set row of every (j, k) so far, or -1
#pragma unroll
    for (int j = 0; j < MAXO; ++j)
#pragma unroll
      for (int k = 0; k < MAXK; ++k) last[j][k] = -1;
    for (int h0 = 0; h0 < g.H; h0 += DOWN_ROWS) {                    // the loads of DOWN_ROWS rows in flight before their stores
      float y[DOWN_ROWS][MAXO];
#pragma unroll
      for (int u = 0; u < DOWN_ROWS; ++u) {
        const int h = h0 + u < g.H ? h0 + u : g.H - 1;               // rows beyond the column read its last pixel, unused
        hist_pixel_values<T, MODE>(g.xf, base + t * g.x.ld_t + ((long long)h * g.W + w) * g.x.ld_p, g.x.ld_c, y[u]);
      }
#pragma unroll
      for (int u = 0; u < DOWN_ROWS; ++u) {
        const int h = h0 + u;
        if (h < g.H) {
#pragma unroll
          for (int j = 0; j < MAXO; ++j) {
            if (j < g.nout) {
#pragma unroll
              for (int k = 0; k < MAXK; ++k) {
                if (k < g.nthr) {
                  last[j][k] = y[u][j] > g.thr[j][k] ? h : last[j][k];
                  G[(long long)(j * g.nthr + k) * P + (long long)h * g.W] = (unsigned short)(last[j][k] >= 0 ? h - last[j][k] : NONE);
                }
              }
            }
          }
        }
      }
    }
  }
}

// upwards, one thread per column of one plane: g read back (0 = a set pixel) and lowered to the distance to the nearest set pixel below
__global__ __launch_bounds__(COL_THREADS) void dist_up_kernel(unsigned short* g, long long nplanes, int H, int W, int njk, int one_series) {
  const int w = blockIdx.x * COL_THREADS + threadIdx.x;
  if (w >= W) return;
  const long long P = (long long)H * W;
  for (long long i = blockIdx.y; i < nplanes; i += gridDim.y) {
    // the planes [t][side][jk] of a pair are one contiguous run; of one series, those of side 0 alone
    const long long plane = one_series ? (i / njk) * 2 * njk + i % njk : i;
    unsigned short* Gp = g + plane * P + w;
    int below = -1;                                                  // the nearest set row at or below h, or -1
    for (int h0 = H - 1; h0 >= 0; h0 -= UP_ROWS) {
      int down[UP_ROWS];
#pragma unroll
      for (int u = 0; u < UP_ROWS; ++u) down[u] = h0 - u >= 0 ? Gp[(long long)(h0 - u) * W] : NONE;
#pragma unroll
      for (int u = 0; u < UP_ROWS; ++u) {
        const int h = h0 - u;
        if (h >= 0) {
          below = down[u] == 0 ? h : below;
          const int up = below >= 0 ? below - h : NONE;
          if (up < down[u]) Gp[(long long)h * W] = (unsigned short)up;
        }
      }
    }
  }
}

struct DistRowArgs {
  const unsigned short* g;
  int H, W, T, nout, nthr, nring, cutoff, paired;
  u64* records;               // [T][nout * nthr][COLS], zeroed before the launch, or NULL
  u64* rings;                 // [nout * nthr][2][nring + 2], accumulated, or NULL
  int* d2;                    // [T][2][nout * nthr][P], or NULL
};

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned a = (unsigned)__shfl_xor((int)v, o, 64);
    v = a > v ? a : v;
  }
  return v;
}

// the exact row minimum of D^2 + g^2[w +- D] at pixel w: s holds g^2 of the row (FAR for none), at least one entry below FAR
__device__ __forceinline__ int dist_scan(const int* s, int w, int W) {
  int best = s[w];
  for (int d = 1; d * d < best; ++d) {
    const int l = w - d, r = w + d;
    if (l < 0 && r >= W) break;
    const int dd = d * d;                                            // dd + FAR < 2^31
    if (l >= 0) { const int c = dd + s[l]; best = c < best ? c : best; }
    if (r < W) { const int c = dd + s[r]; best = c < best ? c : best; }
  }
  return best;
}

__global__ __launch_bounds__(ROW_THREADS) void dist_rows_kernel(DistRowArgs a) {
  __shared__ int sA[DG_DIST_MAX_SIDE], sB[DG_DIST_MAX_SIDE];
  __shared__ unsigned sring[2 * MAXBINS];
  __shared__ int sany[2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int h = blockIdx.x, jk = blockIdx.z;
  const int njk = a.nout * a.nthr, nb = a.nring + 2;
  const long long P = (long long)a.H * a.W;
  const long long row = (long long)h * a.W;
  const long long cap = (long long)a.cutoff * 1024;
  for (int t = blockIdx.y; t < a.T; t += gridDim.y) {                // workgroup-uniform
    __syncthreads();                                                 // the readers of the previous field are done
    if (tid < 2) sany[tid] = 0;
    for (int i = tid; i < 2 * nb; i += ROW_THREADS) sring[i] = 0u;
    __syncthreads();
    const long long plane_a = ((long long)t * 2 * njk + jk) * P, plane_b = plane_a + (long long)njk * P;
    for (int w = tid; w < a.W; w += ROW_THREADS) {
      const int ga = a.g[plane_a + row + w];
      sA[w] = ga == NONE ? FAR : ga * ga;
      if (ga != NONE) sany[0] = 1;
      if (a.paired) {
        const int gb = a.g[plane_b + row + w];
        sB[w] = gb == NONE ? FAR : gb * gb;
        if (gb != NONE) sany[1] = 1;
      }
    }
    __syncthreads();
    const bool hasA = sany[0] != 0, hasB = a.paired && sany[1] != 0, both = hasA && hasB;
    unsigned nA = 0, nB = 0, nAB = 0, maxBA = 0, maxAB = 0;
    u64 dqBA = 0, d2BA = 0, dqAB = 0, d2AB = 0, bad1 = 0, bad2 = 0;
    for (int w = tid; w < a.W; w += ROW_THREADS) {
      const int dA = hasA ? dist_scan(sA, w, a.W) : FAR;
      if (a.d2) a.d2[plane_a + row + w] = dA;
      if (!a.paired) continue;
      const int dB = hasB ? dist_scan(sB, w, a.W) : FAR;
      if (a.d2) a.d2[plane_b + row + w] = dB;
      const bool inA = sA[w] == 0, inB = sB[w] == 0;
      const long long qA = hasA ? dist_dq(dA) : cap, qB = hasB ? dist_dq(dB) : cap;
      const long long wA = qA < cap ? qA : cap, wB = qB < cap ? qB : cap;
      const u64 diff = (u64)(wA > wB ? wA - wB : wB - wA);            // <= 2^19
      bad1 += diff;
      bad2 += diff * diff;
      nA += inA; nB += inB; nAB += inA && inB;
      if (both && inB) { dqBA += (u64)qA; d2BA += (u64)dA; maxBA = (unsigned)dA > maxBA ? (unsigned)dA : maxBA; }
      if (both && inA) { dqAB += (u64)qB; d2AB += (u64)dB; maxAB = (unsigned)dB > maxAB ? (unsigned)dB : maxAB; }
      if (a.rings) {
        if (inB) {
          const int r = hasA ? dist_ring(dA) : a.nring + 1;
          atomicAdd(&sring[hasA && r > a.nring ? a.nring : r], 1u);
        }
        if (inA) {
          const int r = hasB ? dist_ring(dB) : a.nring + 1;
          atomicAdd(&sring[nb + (hasB && r > a.nring ? a.nring : r)], 1u);
        }
      }
    }
    if (!a.paired) continue;                                         // workgroup-uniform
    if (a.records) {
      nA = wave_sum(nA); nB = wave_sum(nB); nAB = wave_sum(nAB);
      bad1 = wave_sum(bad1); bad2 = wave_sum(bad2);
      if (both) {                                                    // workgroup-uniform
        dqBA = wave_sum(dqBA); d2BA = wave_sum(d2BA); maxBA = wave_max(maxBA);
        dqAB = wave_sum(dqAB); d2AB = wave_sum(d2AB); maxAB = wave_max(maxAB);
      }
      if (lane == 0) {
        u64* rec = a.records + ((long long)t * njk + jk) * COLS;
        if (nA) atomicAdd(rec + 0, (u64)nA);
        if (nB) atomicAdd(rec + 1, (u64)nB);
        if (nAB) atomicAdd(rec + 2, (u64)nAB);
        if (dqBA) atomicAdd(rec + 3, dqBA);
        if (d2BA) atomicAdd(rec + 4, d2BA);
        if (maxBA) atomicMax(rec + 5, (u64)maxBA);
        if (dqAB) atomicAdd(rec + 6, dqAB);
        if (d2AB) atomicAdd(rec + 7, d2AB);
        if (maxAB) atomicMax(rec + 8, (u64)maxAB);
        if (bad1) atomicAdd(rec + 9, bad1);
        if (bad2) atomicAdd(rec + 10, bad2);
      }
    }
    if (a.rings) {
      __syncthreads();
      for (int i = tid; i < 2 * nb; i += ROW_THREADS)
        if (sring[i]) atomicAdd(a.rings + (long long)jk * 2 * nb + i, (u64)sring[i]);
    }
  }
}

__global__ __launch_bounds__(ROW_THREADS) void dist_finalize_kernel(u64* records, long long n) {
  const long long i = (long long)blockIdx.x * ROW_THREADS + threadIdx.x;
  if (i >= n) return;
  u64* rec = records + i * COLS;
  if (rec[0] == 0ull || rec[1] == 0ull)
    for (int c = 3; c <= 8; ++c) rec[c] = ~0ull;                     // -1
}

bool spec_ok(const dg_distmap_spec* s, int C) {
  if (!s || s->nthr < 1 || s->nthr > MAXK) return false;
  if (s->nring < 1 || s->nring > DG_DIST_MAX_RINGS || s->cutoff < 1 || s->cutoff > DG_DIST_MAX_CUTOFF) return false;
  return hist_xform_ok(s, C) && hist_thr_ok(s->thr, hist_nout(s, C), s->nthr);
}

bool grid_ok(int H, int W) { return H >= 1 && W >= 1 && H <= DG_DIST_MAX_SIDE && W <= DG_DIST_MAX_SIDE; }

long long planes_of(const dg_eof_fields* a, const dg_distmap_spec* s) {
  return (long long)a->T * 2 * hist_nout(s, a->C) * s->nthr;
}

bool call_ok(const dg_eof_fields* a, int H, int W, const dg_distmap_spec* s) {
  return hist_fields_ok(a) && spec_ok(s, a->C) && grid_ok(H, W) && (long long)H * W == a->P;
}

void cols_of(const dg_eof_fields* x, int side, DistColArgs g, dim3 grid, hipStream_t st) {
  g.x = hist_series(x); g.side = side;
  hist_dispatch<false>(x->dtype, hist_mode(x), [&](auto t, auto m) {
    hipLaunchKernelGGL((dist_down_kernel<decltype(t), decltype(m)::value>), grid, dim3(COL_THREADS), 0, st, g);
  });
}

// Host reference.  hd[r * W + w]: the distance within row r from w to the nearest set pixel of that row (BIG: the row has none).
// d2(h, w) is then the minimum over ALL rows r of (h - r)^2 + hd[r][w]^2; rows are visited outward from h and the visit ends once
// (h - r)^2 alone reaches the best value found, which changes nothing in the minimum.
void host_d2(const std::vector<unsigned char>& M, int H, int W, std::vector<int>& hd, int32_t* out) {
  const int BIG = 1 << 14;                                           // BIG^2 = 2^28: above every real distance, no overflow
  bool any = false;
  for (int r = 0; r < H; ++r) {
    int last = -1;
    for (int w = 0; w < W; ++w) {
      if (M[(size_t)r * W + w]) { last = w; any = true; }
      hd[(size_t)r * W + w] = last >= 0 ? w - last : BIG;
    }
    last = -1;
    for (int w = W - 1; w >= 0; --w) {
      if (M[(size_t)r * W + w]) last = w;
      if (last >= 0 && last - w < hd[(size_t)r * W + w]) hd[(size_t)r * W + w] = last - w;
    }
  }
  for (int h = 0; h < H; ++h) {
    for (int w = 0; w < W; ++w) {
      long long best = FAR;
      if (any) {
        for (int dr = 0; (long long)dr * dr < best && (h - dr >= 0 || h + dr < H); ++dr) {
          for (int sgn = -1; sgn <= 1; sgn += 2) {
            const int r = h + sgn * dr;
            if (r < 0 || r >= H) continue;
            const long long x = hd[(size_t)r * W + w];
            if (x < BIG && (long long)dr * dr + x * x < best) best = (long long)dr * dr + x * x;
          }
        }
      }
      out[(size_t)h * W + w] = (int32_t)best;
    }
  }
}

}  // namespace

extern "C" size_t dg_distmap_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_distmap_spec* s) {
  if (!call_ok(a, H, W, s)) return 0;
  return (size_t)planes_of(a, s) * (size_t)a->P * sizeof(unsigned short);
}

extern "C" int dg_distmap_host_scalars(int32_t d2, int cutoff, int32_t* ring, int64_t* dq, int64_t* w) {
  if (d2 < 0 || d2 > FAR || cutoff < 1 || cutoff > DG_DIST_MAX_CUTOFF || !ring || !dq || !w) return DG_ERR_BAD_ARG;
  const long long cap = (long long)cutoff * 1024, q = dist_dq(d2);
  *ring = dist_ring(d2);
  *dq = q;
  *w = d2 == FAR || q > cap ? cap : q;
  return DG_OK;
}

extern "C" int dg_distmap_host(const dg_distmap_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* records,
                               int64_t* rings, int32_t* d2) {
  if (!spec_ok(s, C) || !a || !grid_ok(H, W)) return DG_ERR_BAD_ARG;
  if (b ? (!records && !rings && !d2) : (!d2 || records || rings)) return DG_ERR_BAD_ARG;
  const int nout = hist_nout(s, C), nb = s->nring + 2;
  const size_t P = (size_t)H * W;
  const long long cap = (long long)s->cutoff * 1024;
  const float* x[2] = {a, b};
  std::vector<float> y(P);
  std::vector<unsigned char> mask[2];
  std::vector<int32_t> dist[2];
  std::vector<int> hd(P);
  for (int j = 0; j < nout; ++j) {
    for (int k = 0; k < s->nthr; ++k) {
      long long n[2] = {0, 0};
      for (int e = 0; e < (b ? 2 : 1); ++e) {
        for (size_t p = 0; p < P; ++p) y[p] = hist_host_value(s, x[e], C, P, p, j);
        mask[e].assign(P, 0);
        for (size_t p = 0; p < P; ++p) {
          mask[e][p] = y[p] > s->thr[j][k] ? 1 : 0;
          n[e] += mask[e][p];
        }
        dist[e].resize(P);
        host_d2(mask[e], H, W, hd, dist[e].data());
        if (d2) std::copy(dist[e].begin(), dist[e].end(), d2 + (((size_t)e * nout + j) * s->nthr + k) * P);
      }
      if (!b) continue;
      const bool both = n[0] > 0 && n[1] > 0;
      long long rec[COLS] = {n[0], n[1], 0, 0, 0, 0, 0, 0, 0, 0, 0};
      int64_t* ring = rings ? rings + ((size_t)j * s->nthr + k) * 2 * nb : nullptr;
      for (size_t p = 0; p < P; ++p) {
        const bool in[2] = {mask[0][p] != 0, mask[1][p] != 0};
        long long wv[2];
        for (int e = 0; e < 2; ++e) {
          const long long q = n[e] > 0 ? dist_dq(dist[e][p]) : cap;
          wv[e] = q < cap ? q : cap;
        }
        const long long diff = wv[0] > wv[1] ? wv[0] - wv[1] : wv[1] - wv[0];
        rec[9] += diff;
        rec[10] += diff * diff;
        rec[2] += in[0] && in[1];
        for (int dir = 0; dir < 2; ++dir) {                          // dir 0: the pixels of B by their distance to A; 1: of A to B
          const int from = 1 - dir, to = dir;
          if (!in[from]) continue;
          const int32_t d = dist[to][p];
          if (both) {
            rec[3 + 3 * dir] += dist_dq(d);
            rec[4 + 3 * dir] += d;
            if (d > rec[5 + 3 * dir]) rec[5 + 3 * dir] = d;
          }
          if (ring) {
            const int r = n[to] > 0 ? dist_ring(d) : s->nring + 1;
            ring[(size_t)dir * nb + (n[to] > 0 && r > s->nring ? s->nring : r)] += 1;
          }
        }
      }
      if (!both)
        for (int c = 3; c <= 8; ++c) rec[c] = -1;
      if (records) std::copy(rec, rec + COLS, records + ((size_t)j * s->nthr + k) * COLS);
    }
  }
  return DG_OK;
}

extern "C" int dg_distmap(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_distmap_spec* s, void* ws,
                          int64_t* records, int64_t* rings, int32_t* d2, void* stream) {
  if (!call_ok(a, H, W, s) || !ws) return DG_ERR_BAD_ARG;
  if (b && (!hist_fields_ok(b) || b->T != a->T || b->C != a->C || b->P != a->P)) return DG_ERR_BAD_ARG;
  if (b ? (!records && !rings && !d2) : (!d2 || records || rings)) return DG_ERR_BAD_ARG;
  if ((a->dtype != DG_F32 && a->dtype != DG_BF16) || (b && b->dtype != DG_F32 && b->dtype != DG_BF16)) return DG_ERR_BAD_DTYPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nout = hist_nout(s, a->C), njk = nout * s->nthr;
  const long long nrec = (long long)a->T * njk;
  if (records && hipMemsetAsync(records, 0, (size_t)nrec * COLS * sizeof(int64_t), st) != hipSuccess) return DG_ERR_LAUNCH;

  DistColArgs g;
  g.xf = hist_xform(s, a->C);
  g.H = H; g.W = W; g.T = a->T; g.nout = nout; g.nthr = s->nthr;
  hist_thr_pad(s->thr, nout, s->nthr, g.thr);
  g.g = reinterpret_cast<unsigned short*>(ws);
  const unsigned gt = (unsigned)(a->T < DIST_GRID_T ? a->T : DIST_GRID_T);
  const dim3 cgrid((unsigned)((W + COL_THREADS - 1) / COL_THREADS), gt);
  cols_of(a, 0, g, cgrid, st);
  if (b) cols_of(b, 1, g, cgrid, st);
  const long long nup = (long long)a->T * njk * (b ? 2 : 1);
  hipLaunchKernelGGL(dist_up_kernel, dim3(cgrid.x, (unsigned)(nup < DIST_GRID_PLANES ? nup : DIST_GRID_PLANES)), dim3(COL_THREADS), 0, st,
                     g.g, nup, H, W, njk, b ? 0 : 1);

  DistRowArgs r;
  r.g = g.g; r.H = H; r.W = W; r.T = a->T; r.nout = nout; r.nthr = s->nthr; r.nring = s->nring; r.cutoff = s->cutoff;
  r.paired = b ? 1 : 0;
  r.records = reinterpret_cast<u64*>(records); r.rings = reinterpret_cast<u64*>(rings); r.d2 = d2;
  hipLaunchKernelGGL(dist_rows_kernel, dim3((unsigned)H, gt, (unsigned)njk), dim3(ROW_THREADS), 0, st, r);
  if (records)
    hipLaunchKernelGGL(dist_finalize_kernel, dim3((unsigned)((nrec + ROW_THREADS - 1) / ROW_THREADS)), dim3(ROW_THREADS), 0, st,
                       reinterpret_cast<u64*>(records), nrec);
  return dg_check_launch();
}
