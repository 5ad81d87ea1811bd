// Value histograms (include/downgan_hip.h "Value histograms") of fields read through the EOF descriptor (NCHW, [n, H, W, c],
// padded NHWC; fp32 / bf16), any T and P.
//   hist_kernel<T, MODE>   grid-stride over the items (t, pixel group) of a fixed share per workgroup: affine, speed, bin rule,
//                          LDS histogram (ds_add_u32), per-thread fp64 moments and fp32 extrema; then the non-zero bins are
//                          added to counts with 64-bit integer atomics and the moments / extrema of the workgroup are stored
//                          to its slot of the workspace (lane order, then wave order: fixed)
//   hist_finish_kernel     one workgroup per output channel: the slots summed in workgroup order (fixed), += moments,
//                          min / max into extrema
// MODE: HIST_NCHW4 = four consecutive pixels of one NCHW plane per load (16 B fp32, 8 B bf16); HIST_PIX16 = one 16-byte
// load per pixel (the generator's [B, H, W, 16] bf16 output: 8 channels); HIST_ANY = one element per load (any strides).
// Every fp32 operation of the definition is one rounded operation (no contraction, no fast-math sqrt); integer counts do not
// depend on arrival order, and nothing else is summed by atomics, so two calls are bit-identical.
#include <float.h>
#include <math.h>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_GRID_MAX = 2048;                   // workgroups per launch (memory-bound: cap and grid-stride)
constexpr long long HIST_ITEMS_MAX = 1LL << 20;       // items per thread per launch: <= 2^30 values per workgroup, no uint32 wrap
constexpr int MAXC = DG_EOF_MAX_C, MAXO = DG_HIST_MAX_OUT;

struct HistArgs {
  HistSeries x;
  HistXform xf;
  int P, nbins;
  long long t0, items;        // fields t0 .. of this launch; items = fields * items per field
  int ipf;                    // items per field
  float lo[MAXO], inv_w[MAXO];
  unsigned long long* counts; // int64 [nout][nbins + 3]
  double* part_m;             // [grid][MAXO][2]
  float* part_e;              // [grid][MAXO][2]
};

struct Acc {
  double s1, s2;
  float mn, mx;
  __device__ void init() { s1 = 0.0; s2 = 0.0; mn = INFINITY; mx = -INFINITY; }
  __device__ __forceinline__ void add(float y) {
    const bool fin = fabsf(y) <= FLT_MAX;                       // false for NaN and +-inf
    const double d = fin ? (double)y : 0.0;
    s1 += d;
    s2 += d * d;                                                // exact product (24-bit mantissas)
    mn = fin ? fminf(mn, y) : mn;
    mx = fin ? fmaxf(mx, y) : mx;
  }
};

template <typename T, int MODE>
__global__ __launch_bounds__(HIST_THREADS) void hist_kernel(HistArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned int hist_lds[];    // [nout][nbins + 3]
  __shared__ double red_m[HIST_THREADS / 64][MAXO][2];
  __shared__ float red_e[HIST_THREADS / 64][MAXO][2];
  const HistXform& xf = a.xf;
  const int nb3 = a.nbins + 3, nout = xf.C + xf.speed;
  for (int i = threadIdx.x; i < nout * nb3; i += HIST_THREADS) hist_lds[i] = 0u;
  __syncthreads();
  Acc acc[MAXO];
#pragma unroll
  for (int j = 0; j < MAXO; ++j) acc[j].init();
  constexpr int NPX = MODE == HIST_NCHW4 ? 4 : 1;
  // item g = (field t0 + t, item i of the field); the stride is split once so that the loop does no 64-bit division
  const long long stride = (long long)gridDim.x * HIST_THREADS, g0 = (long long)blockIdx.x * HIST_THREADS + threadIdx.x;
  const long long dt = stride / a.ipf, di = stride % a.ipf;
  long long t = a.t0 + g0 / a.ipf, i = g0 % a.ipf;
  for (long long g = g0; g < a.items; g += stride) {
    float v[4][MAXC];
    hist_load_item<T, MODE>(a.x, xf.C, t, i, v);
    t += dt;
    i += di;
    if (i >= a.ipf) { i -= a.ipf; ++t; }
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      float yu = 0.f, yv = 0.f;
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        if (c < xf.C) {
          const float y = hist_affine(v[k][c], xf.scale[c], xf.offset[c]);
          atomicAdd(&hist_lds[c * nb3 + hist_bin(y, a.lo[c], a.inv_w[c], a.nbins)], 1u);
          acc[c].add(y);
          yu = c == xf.su ? y : yu;
          yv = c == xf.sv ? y : yv;
        }
      }
      if (xf.speed) {
        const float s = hist_speed(yu, yv);
        atomicAdd(&hist_lds[xf.C * nb3 + hist_bin(s, a.lo[xf.C], a.inv_w[xf.C], a.nbins)], 1u);
        acc[MAXO - 1].add(s);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nout * nb3; i += HIST_THREADS) {
    const unsigned n = hist_lds[i];
    if (n) atomicAdd(a.counts + i, (unsigned long long)n);
  }
  // moments / extrema: butterfly over the wave (the same order in every lane), then the waves in order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < MAXO; ++j) {
    for (int m = 32; m >= 1; m >>= 1) {
      acc[j].s1 += hist_shfl_xor_f64(acc[j].s1, m);
      acc[j].s2 += hist_shfl_xor_f64(acc[j].s2, m);
      acc[j].mn = fminf(acc[j].mn, __shfl_xor(acc[j].mn, m, 64));
      acc[j].mx = fmaxf(acc[j].mx, __shfl_xor(acc[j].mx, m, 64));
    }
    if (lane == 0) {
      red_m[wave][j][0] = acc[j].s1; red_m[wave][j][1] = acc[j].s2;
      red_e[wave][j][0] = acc[j].mn; red_e[wave][j][1] = acc[j].mx;
    }
  }
  __syncthreads();
  if (threadIdx.x < MAXO) {
    const int j = threadIdx.x;                                  // slot j: component j, or the speed at MAXO - 1
    double s1 = 0.0, s2 = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int w = 0; w < HIST_THREADS / 64; ++w) {
      s1 += red_m[w][j][0]; s2 += red_m[w][j][1];
      mn = fminf(mn, red_e[w][j][0]); mx = fmaxf(mx, red_e[w][j][1]);
    }
    double* pm = a.part_m + ((long long)blockIdx.x * MAXO + j) * 2;
    float* pe = a.part_e + ((long long)blockIdx.x * MAXO + j) * 2;
    pm[0] = s1; pm[1] = s2; pe[0] = mn; pe[1] = mx;
  }
}

// one workgroup per output channel: thread i sums the slots i, i + 256, ... in order, then a fixed tree over the threads
__global__ __launch_bounds__(HIST_THREADS) void hist_finish_kernel(const double* part_m, const float* part_e, int grid, int C,
                                                                   double* moments, float* extrema) {
  __shared__ double sm[HIST_THREADS][2];
  __shared__ float se[HIST_THREADS][2];
  const int j = blockIdx.x;                                     // output channel
  const int slot = j < C ? j : MAXO - 1;
  double s1 = 0.0, s2 = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int g = threadIdx.x; g < grid; g += HIST_THREADS) {
    const long long o = ((long long)g * MAXO + slot) * 2;
    s1 += part_m[o]; s2 += part_m[o + 1];
    mn = fminf(mn, part_e[o]); mx = fmaxf(mx, part_e[o + 1]);
  }
  sm[threadIdx.x][0] = s1; sm[threadIdx.x][1] = s2;
  se[threadIdx.x][0] = mn; se[threadIdx.x][1] = mx;
  __syncthreads();
  for (int h = HIST_THREADS / 2; h >= 1; h >>= 1) {
    if (threadIdx.x < h) {
      sm[threadIdx.x][0] += sm[threadIdx.x + h][0];
      sm[threadIdx.x][1] += sm[threadIdx.x + h][1];
      se[threadIdx.x][0] = fminf(se[threadIdx.x][0], se[threadIdx.x + h][0]);
      se[threadIdx.x][1] = fmaxf(se[threadIdx.x][1], se[threadIdx.x + h][1]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    moments[2 * j] += sm[0][0];
    moments[2 * j + 1] += sm[0][1];
    extrema[2 * j] = fminf(extrema[2 * j], se[0][0]);
    extrema[2 * j + 1] = fmaxf(extrema[2 * j + 1], se[0][1]);
  }
}

bool spec_ok(const dg_hist_spec* s, int C) {
  if (!s || s->nbins < 1 || s->nbins > DG_HIST_MAX_BINS || !hist_xform_ok(s, C)) return false;
  for (int j = 0; j < hist_nout(s, C); ++j)
    if (!hist_finite(s->lo[j]) || !(s->inv_w[j] > 0.f && s->inv_w[j] <= FLT_MAX)) return false;
  return true;
}

int hist_grid(long long items) {
  const long long g = (items + HIST_THREADS - 1) / HIST_THREADS;
  return (int)(g < 1 ? 1 : g > HIST_GRID_MAX ? HIST_GRID_MAX : g);
}

template <typename T, int MODE>
int launch(const HistArgs& a, int grid, size_t lds, hipStream_t st) {
  DG_SET_MAX_LDS_ONCE((hist_kernel<T, MODE>), (int)(MAXO * (DG_HIST_MAX_BINS + 3) * sizeof(unsigned)));
  hipLaunchKernelGGL((hist_kernel<T, MODE>), dim3(grid), dim3(HIST_THREADS), lds, st, a);
  return DG_OK;
}

}  // namespace

extern "C" size_t dg_hist_ws_bytes(const dg_eof_fields* x, const dg_hist_spec* s) {
  if (!hist_fields_ok(x) || !spec_ok(s, x->C)) return 0;
  return (size_t)HIST_GRID_MAX * MAXO * 2 * (sizeof(double) + sizeof(float));
}

extern "C" int dg_hist_host_bins(const dg_hist_spec* s, const float* x, int C, int64_t n, int32_t* bins) {
  if (!spec_ok(s, C) || n < 0 || (n > 0 && (!x || !bins))) return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C);
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < nout; ++j)
      bins[(int64_t)j * n + i] = hist_bin(hist_host_value(s, x, C, (size_t)n, (size_t)i, j), s->lo[j], s->inv_w[j], s->nbins);
  return DG_OK;
}

extern "C" int dg_hist(const dg_eof_fields* x, const dg_hist_spec* s, void* ws, int64_t* counts, double* moments, float* extrema,
                       void* stream) {
  if (!hist_fields_ok(x) || !spec_ok(s, x->C) || !ws || !counts || !moments || !extrema) return DG_ERR_BAD_SHAPE;
  if (x->dtype != DG_F32 && x->dtype != DG_BF16) return DG_ERR_BAD_DTYPE;
  const int mode = hist_mode(x);
  const int nout = hist_nout(s, x->C);
  HistArgs a;
  a.x = hist_series(x);
  a.xf = hist_xform(s, x->C);
  a.P = x->P; a.nbins = s->nbins;
  a.ipf = mode == HIST_NCHW4 ? x->P / 4 : x->P;
  for (int j = 0; j < MAXO; ++j) {
    a.lo[j] = j < nout ? s->lo[j] : 0.f;
    a.inv_w[j] = j < nout ? s->inv_w[j] : 1.f;
  }
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.part_m = reinterpret_cast<double*>(ws);
  a.part_e = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + (size_t)HIST_GRID_MAX * MAXO * 2 * sizeof(double));
  const size_t lds = (size_t)nout * (s->nbins + 3) * sizeof(unsigned);
  // fields per launch: at most HIST_ITEMS_MAX items per thread, so no workgroup's uint32 bin can wrap
  const long long tmax = (long long)HIST_GRID_MAX * HIST_THREADS * HIST_ITEMS_MAX / a.ipf;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (long long t0 = 0; t0 < x->T; t0 += tmax) {
    const long long nt = x->T - t0 < tmax ? x->T - t0 : tmax;
    a.t0 = t0;
    a.items = nt * a.ipf;
    const int grid = hist_grid(a.items);
    // t, m: tags of the element type and the load mode (hist_common.h "dtype x load mode"): decltype(m)::value is the HIST_* constant
    const int rc = hist_dispatch(x->dtype, mode, [&](auto t, auto m) { return launch<decltype(t), decltype(m)::value>(a, grid, lds, st); });
    if (rc != DG_OK) return rc;
    hipLaunchKernelGGL(hist_finish_kernel, dim3(nout), dim3(HIST_THREADS), 0, st, (const double*)a.part_m, (const float*)a.part_e,
                       grid, x->C, moments, extrema);
  }
  return dg_check_launch();
}
