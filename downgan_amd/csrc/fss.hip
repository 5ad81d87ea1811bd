// Fractions skill score (include/downgan_hip.h "Fractions skill score") of two series of H x W fields read through the EOF
// descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16): for every output channel j, threshold k and window side n the
// exact integers D = sum (c_a - c_b)^2, A = sum c_a^2, B = sum c_b^2 of the window counts of the exceedance masks.
//   fss_rows_kernel<T, MODE>   one wave per row (t, h) of one series: 64 pixels per step, the output values y of hist_common.h,
//                              the masks of all (j, k) as wave ballots, the inclusive row prefix count of each lane by popcount
//                              plus the row's running count (wave-uniform) -> plane (t, series, j, k) of the workspace, uint32
//   fss_cols_kernel            one thread per (plane, column): the running sum down the rows, in place (coalesced over the
//                              columns) -> summed-area tables, entries <= P <= 2^22
//   fss_windows_kernel         workgroup = 1024 pixels of one (t, j, k): per pixel and scale the four clipped corners of both
//                              tables, c_a and c_b, squares in 64-bit; wave shuffles, then LDS over the waves, then one 64-bit
//                              integer atomic add per (scale, term) into the field's slot of the workspace
//   fss_finish_kernel          sums += the slots over t (and the slots copied to per_field), rates += the last entry of every
//                              table (= the number of set mask pixels)
// MODE: HIST_PIX16 = one 16-byte load per pixel (the generator's [B, H, W, 16] bf16 output), HIST_ANY = one element per load
// (NCHW planes too: a wave's 64 pixels are consecutive, so the loads coalesce).  No float after the compare, integer atomics
// only: exact, and two calls on the same data are bit-identical.
#include <float.h>
#include <math.h>

#include <vector>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int FSS_THREADS = 256;
constexpr int FSS_WAVES = FSS_THREADS / 64;
constexpr int FSS_PIX_PER_WG = 1024;                  // 4 pixels per thread: 1024 c^2 <= 2^54 per workgroup sum
constexpr int FSS_GRID_T = 4096;                      // fields across gridDim.y at most; the kernels stride over the rest
constexpr int FSS_COLS_GRID_MAX = 1 << 20;
constexpr int MAXO = DG_HIST_MAX_OUT, MAXK = DG_FSS_MAX_THR, MAXS = DG_FSS_MAX_SCALES;
constexpr long long FSS_LIMIT = 1LL << 62;

typedef unsigned long long u64;

struct FssRowArgs {
  HistSeries x;
  HistXform xf;
  int H, W, T, nout, nthr, side;
  float thr[MAXO][MAXK];
  unsigned* planes;           // plane ((t * 2 + side) * nout + j) * nthr + k, H * W entries each
};

struct FssWinArgs {
  const unsigned* planes;
  u64* slots;                 // [T][nout][nthr][nscale][3]
  int H, W, T, nout, nthr, nscale;
  int r[MAXS];
};

template <typename T, int MODE>
__global__ __launch_bounds__(FSS_THREADS) void fss_rows_kernel(FssRowArgs g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.x * FSS_WAVES + wave;
  if (h >= g.H) return;                                              // wave-uniform
  const long long P = (long long)g.H * g.W;
  const T* base = reinterpret_cast<const T*>(g.x.base);
  const u64 upto = ~0ull >> (63 - lane);                             // lanes 0 .. lane
  for (int t = blockIdx.y; t < g.T; t += gridDim.y) {
    unsigned carry[MAXO][MAXK];
#pragma unroll
    for (int j = 0; j < MAXO; ++j)
#pragma unroll
      for (int k = 0; k < MAXK; ++k) carry[j][k] = 0u;
    unsigned* field = g.planes + ((long long)t * 2 + g.side) * g.nout * g.nthr * P + (long long)h * g.W;
    for (int w0 = 0; w0 < g.W; w0 += 64) {
      const int w = w0 + lane;
      const bool in = w < g.W;
      const long long p = (long long)h * g.W + (in ? w : g.W - 1);   // lanes beyond the row read its last pixel, unused
      float y[MAXO];
      hist_pixel_values<T, MODE>(g.xf, base + t * g.x.ld_t + p * g.x.ld_p, g.x.ld_c, y);
#pragma unroll
      for (int j = 0; j < MAXO; ++j) {
        if (j < g.nout) {
#pragma unroll
          for (int k = 0; k < MAXK; ++k) {
            if (k < g.nthr) {
              const u64 m = __ballot(in && y[j] > g.thr[j][k]);
              if (in) field[(long long)(j * g.nthr + k) * P + w] = carry[j][k] + (unsigned)__popcll(m & upto);
              carry[j][k] += (unsigned)__popcll(m);
            }
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(FSS_THREADS) void fss_cols_kernel(unsigned* planes, long long nplanes, int H, int W) {
  const long long total = nplanes * W, stride = (long long)gridDim.x * FSS_THREADS, P = (long long)H * W;
  for (long long i = (long long)blockIdx.x * FSS_THREADS + threadIdx.x; i < total; i += stride) {
    unsigned* q = planes + (i / W) * P + (i % W);
    unsigned acc = 0u;
    int h = 0;
    for (; h + 8 <= H; h += 8) {
      unsigned v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = q[(long long)(h + u) * W];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc += v[u];
        q[(long long)(h + u) * W] = acc;
      }
    }
    for (; h < H; ++h) {
      acc += q[(long long)h * W];
      q[(long long)h * W] = acc;
    }
  }
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}

// the number of set mask pixels in rows h0 + 1 .. h1, columns w0 + 1 .. w1 of the table s (h0, w0 = -1: from the border)
__device__ __forceinline__ unsigned fss_box(const unsigned* s, int W, int h0, int h1, int w0, int w1) {
  const unsigned* top = s + (long long)(h0 < 0 ? 0 : h0) * W;
  const unsigned* bot = s + (long long)h1 * W;
  const unsigned br = bot[w1];
  const unsigned bl = w0 >= 0 ? bot[w0] : 0u;
  const unsigned tr = h0 >= 0 ? top[w1] : 0u;
  const unsigned tl = h0 >= 0 && w0 >= 0 ? top[w0] : 0u;
  return br - bl - tr + tl;
}

__global__ __launch_bounds__(FSS_THREADS) void fss_windows_kernel(FssWinArgs g) {
  __shared__ u64 red[FSS_WAVES][MAXS][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jk = blockIdx.z, njk = g.nout * g.nthr;
  const long long P = (long long)g.H * g.W;
  for (int t = blockIdx.y; t < g.T; t += gridDim.y) {                // workgroup-uniform
    const unsigned* sa = g.planes + (((long long)t * 2) * njk + jk) * P;
    const unsigned* sb = g.planes + (((long long)t * 2 + 1) * njk + jk) * P;
    u64 acc[MAXS][3];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) acc[s][0] = acc[s][1] = acc[s][2] = 0ull;
    for (int u = 0; u < FSS_PIX_PER_WG / FSS_THREADS; ++u) {
      const long long p = (long long)blockIdx.x * FSS_PIX_PER_WG + u * FSS_THREADS + threadIdx.x;
      if (p < P) {
        const int h = (int)(p / g.W), w = (int)(p % g.W);
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
          if (s < g.nscale) {
            const int r = g.r[s];
            const int h0 = (h - r < 0 ? 0 : h - r) - 1, h1 = h + r > g.H - 1 ? g.H - 1 : h + r;
            const int w0 = (w - r < 0 ? 0 : w - r) - 1, w1 = w + r > g.W - 1 ? g.W - 1 : w + r;
            const u64 ca = fss_box(sa, g.W, h0, h1, w0, w1), cb = fss_box(sb, g.W, h0, h1, w0, w1);
            const u64 d = ca > cb ? ca - cb : cb - ca;
            acc[s][0] += d * d;
            acc[s][1] += ca * ca;
            acc[s][2] += cb * cb;
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      if (s < g.nscale) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const u64 v = wave_sum_u64(acc[s][e]);
          if (lane == 0) red[wave][s][e] = v;
        }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < g.nscale * 3) {
      const int s = threadIdx.x / 3, e = threadIdx.x % 3;
      u64 v = 0ull;
      for (int q = 0; q < FSS_WAVES; ++q) v += red[q][s][e];
      if (v) atomicAdd(g.slots + (((long long)t * njk + jk) * g.nscale + s) * 3 + e, v);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(FSS_THREADS) void fss_finish_kernel(const u64* slots, const unsigned* planes, int T, int njk, int nscale,
                                                                 long long P, u64* sums, u64* rates, u64* per_field) {
  const int n = njk * nscale * 3, stride = gridDim.x * FSS_THREADS, i0 = blockIdx.x * FSS_THREADS + threadIdx.x;
  for (int i = i0; i < n; i += stride) {
    u64 total = 0ull;
    for (int t = 0; t < T; ++t) {
      const u64 v = slots[(long long)t * n + i];
      total += v;
      if (per_field) per_field[(long long)t * n + i] = v;
    }
    sums[i] += total;
  }
  for (int i = i0; i < njk * 2; i += stride) {
    const int jk = i / 2, side = i % 2;
    u64 total = 0ull;
    for (int t = 0; t < T; ++t) total += planes[(((long long)t * 2 + side) * njk + jk) * P + P - 1];
    rates[i] += total;
  }
}

bool spec_ok(const dg_fss_spec* s, int C) {
  if (!s || s->nthr < 1 || s->nthr > MAXK || s->nscale < 1 || s->nscale > MAXS) return false;
  if (!hist_xform_ok(s, C) || !hist_thr_ok(s->thr, hist_nout(s, C), s->nthr)) return false;
  for (int i = 0; i < s->nscale; ++i) {
    const int n = s->win[i];
    if (n < 1 || n > 2 * DG_FSS_MAX_SIDE - 1 || n % 2 == 0 || (i > 0 && n <= s->win[i - 1])) return false;
  }
  return true;
}

long long bound_of(int H, int W, int win) {
  if (H < 1 || W < 1 || H > DG_FSS_MAX_SIDE || W > DG_FSS_MAX_SIDE || win < 1 || win > 2 * DG_FSS_MAX_SIDE - 1 || win % 2 == 0) return 0;
  const unsigned __int128 box = (unsigned __int128)(win < H ? win : H) * (unsigned)(win < W ? win : W);
  const unsigned __int128 v = (unsigned __int128)H * (unsigned)W * box * box;
  return v > (unsigned __int128)FSS_LIMIT ? 0 : (long long)v;
}

// the largest dg_fss_bound of the spec's scales on this grid; 0 when the grid or one of the scales is not admissible
long long max_bound(int H, int W, const dg_fss_spec* s) {
  long long m = 0;
  for (int i = 0; i < s->nscale; ++i) {
    const long long b = bound_of(H, W, s->win[i]);
    if (b == 0) return 0;
    m = b > m ? b : m;
  }
  return m;
}

struct Layout {
  int nout, njk;
  size_t slot_bytes, bytes;
};

Layout layout_of(const dg_eof_fields* a, const dg_fss_spec* s) {
  Layout l;
  l.nout = hist_nout(s, a->C);
  l.njk = l.nout * s->nthr;
  l.slot_bytes = hist_round256((size_t)a->T * l.njk * s->nscale * 3 * sizeof(u64));
  l.bytes = l.slot_bytes + (size_t)a->T * 2 * l.njk * (size_t)a->P * sizeof(unsigned);
  return l;
}

bool call_ok(const dg_eof_fields* a, int H, int W, const dg_fss_spec* s) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C)) return false;
  if (H < 1 || W < 1 || H > DG_FSS_MAX_SIDE || W > DG_FSS_MAX_SIDE || (long long)H * W != a->P) return false;
  const long long mb = max_bound(H, W, s);
  return mb > 0 && a->T <= FSS_LIMIT / mb;                         // T * max_s bound <= 2^62: one call cannot overflow
}

void rows_of(const dg_eof_fields* x, int side, FssRowArgs g, dim3 grid, hipStream_t st) {
  g.x = hist_series(x); g.side = side;
  hist_dispatch<false>(x->dtype, hist_mode(x), [&](auto t, auto m) {
    hipLaunchKernelGGL((fss_rows_kernel<decltype(t), decltype(m)::value>), grid, dim3(FSS_THREADS), 0, st, g);
  });
}

}  // namespace

extern "C" int64_t dg_fss_bound(int H, int W, int win) { return bound_of(H, W, win); }

extern "C" size_t dg_fss_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_fss_spec* s) {
  if (!call_ok(a, H, W, s)) return 0;
  return layout_of(a, s).bytes;
}

extern "C" int dg_fss_host(const dg_fss_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* sums, int64_t* rates) {
  if (!spec_ok(s, C) || !a || !b || !sums || !rates || H < 1 || W < 1 || H > DG_FSS_MAX_SIDE || W > DG_FSS_MAX_SIDE) return DG_ERR_BAD_SHAPE;
  if (max_bound(H, W, s) == 0) return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C);
  const size_t P = (size_t)H * W, W1 = (size_t)W + 1;
  std::vector<int64_t> sat[2];                                       // (H + 1) x (W + 1), a zero row and column in front
  sat[0].assign((size_t)(H + 1) * W1, 0);
  sat[1].assign((size_t)(H + 1) * W1, 0);
  const float* x[2] = {a, b};
  for (int j = 0; j < nout; ++j) {
    for (int k = 0; k < s->nthr; ++k) {
      for (int side = 0; side < 2; ++side) {
        for (int h = 0; h < H; ++h) {
          int64_t row = 0;
          for (int w = 0; w < W; ++w) {
            const size_t p = (size_t)h * W + w;
            row += hist_host_value(s, x[side], C, P, p, j) > s->thr[j][k] ? 1 : 0;
            sat[side][(size_t)(h + 1) * W1 + w + 1] = sat[side][(size_t)h * W1 + w + 1] + row;
          }
        }
        rates[(j * s->nthr + k) * 2 + side] += sat[side][(size_t)H * W1 + W];
      }
      for (int i = 0; i < s->nscale; ++i) {
        const int r = s->win[i] / 2;
        int64_t D = 0, A = 0, B = 0;
        for (int h = 0; h < H; ++h) {
          const size_t h0 = h - r < 0 ? 0 : h - r, h1 = (h + r > H - 1 ? H - 1 : h + r) + 1;
          for (int w = 0; w < W; ++w) {
            const size_t w0 = w - r < 0 ? 0 : w - r, w1 = (w + r > W - 1 ? W - 1 : w + r) + 1;
            int64_t c[2];
            for (int side = 0; side < 2; ++side) {
              const std::vector<int64_t>& S = sat[side];
              c[side] = S[h1 * W1 + w1] - S[h0 * W1 + w1] - S[h1 * W1 + w0] + S[h0 * W1 + w0];
            }
            D += (c[0] - c[1]) * (c[0] - c[1]);
            A += c[0] * c[0];
            B += c[1] * c[1];
          }
        }
        int64_t* o = sums + ((size_t)(j * s->nthr + k) * s->nscale + i) * 3;
        o[0] += D; o[1] += A; o[2] += B;
      }
    }
  }
  return DG_OK;
}

extern "C" int dg_fss(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_fss_spec* s, void* ws, int64_t* sums,
                      int64_t* rates, int64_t* per_field, void* stream) {
  if (!call_ok(a, H, W, s) || !hist_fields_ok(b) || b->T != a->T || b->C != a->C || b->P != a->P || !ws || !sums || !rates)
    return DG_ERR_BAD_SHAPE;
  if ((a->dtype != DG_F32 && a->dtype != DG_BF16) || (b->dtype != DG_F32 && b->dtype != DG_BF16)) return DG_ERR_BAD_DTYPE;
  const Layout l = layout_of(a, s);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  u64* slots = reinterpret_cast<u64*>(ws);
  unsigned* planes = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ws) + l.slot_bytes);
  if (hipMemsetAsync(slots, 0, l.slot_bytes, st) != hipSuccess) return DG_ERR_LAUNCH;

  FssRowArgs g;
  g.xf = hist_xform(s, a->C);
  g.H = H; g.W = W; g.T = a->T; g.nout = l.nout; g.nthr = s->nthr;
  hist_thr_pad(s->thr, l.nout, s->nthr, g.thr);
  g.planes = planes;
  const unsigned gt = (unsigned)(a->T < FSS_GRID_T ? a->T : FSS_GRID_T);
  const dim3 rgrid((unsigned)((H + FSS_WAVES - 1) / FSS_WAVES), gt);
  rows_of(a, 0, g, rgrid, st);
  rows_of(b, 1, g, rgrid, st);

  const long long nplanes = (long long)a->T * 2 * l.njk;
  long long cg = (nplanes * W + FSS_THREADS - 1) / FSS_THREADS;
  cg = cg > FSS_COLS_GRID_MAX ? FSS_COLS_GRID_MAX : cg;
  hipLaunchKernelGGL(fss_cols_kernel, dim3((unsigned)cg), dim3(FSS_THREADS), 0, st, planes, nplanes, H, W);

  FssWinArgs wa;
  wa.planes = planes; wa.slots = slots; wa.H = H; wa.W = W; wa.T = a->T; wa.nout = l.nout; wa.nthr = s->nthr; wa.nscale = s->nscale;
  for (int i = 0; i < MAXS; ++i) wa.r[i] = i < s->nscale ? s->win[i] / 2 : 0;
  const dim3 wgrid((unsigned)(((long long)a->P + FSS_PIX_PER_WG - 1) / FSS_PIX_PER_WG), gt, (unsigned)l.njk);
  hipLaunchKernelGGL(fss_windows_kernel, wgrid, dim3(FSS_THREADS), 0, st, wa);

  const int n = l.njk * s->nscale * 3;
  hipLaunchKernelGGL(fss_finish_kernel, dim3((unsigned)((n + FSS_THREADS - 1) / FSS_THREADS)), dim3(FSS_THREADS), 0, st,
                     (const u64*)slots, (const unsigned*)planes, a->T, l.njk, s->nscale, (long long)a->P,
                     reinterpret_cast<u64*>(sums), reinterpret_cast<u64*>(rates), reinterpret_cast<u64*>(per_field));
  return dg_check_launch();
}
