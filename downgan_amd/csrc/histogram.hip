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
  const void* base;
  long long ld_t, ld_c, ld_p;
  int C, P, nbins, speed, su, sv;
  long long t0, items;        // fields t0 .. of this launch; items = fields * items per field
  int ipf;                    // items per field
  float lo[MAXO], inv_w[MAXO], scale[MAXC], offset[MAXC];
  unsigned long long* counts; // int64 [nout][nbins + 3]
  double* part_m;             // [grid][MAXO][2]
  float* part_e;              // [grid][MAXO][2]
};

__device__ __forceinline__ double shfl_xor_d(double v, int m) {
  return __longlong_as_double(__shfl_xor(__double_as_longlong(v), m, 64));
}

template <typename T, int MODE>
__device__ __forceinline__ void load_item(const HistArgs& a, long long t, long long i, float (&v)[4][MAXC]) {
  const T* base = reinterpret_cast<const T*>(a.base);
  if (MODE == HIST_NCHW4) {
    const T* q = base + t * a.ld_t + 4 * i;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < a.C) {
        float w[4];
        ld4(q + c * a.ld_c, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k][c] = w[k];
      }
    }
  } else if (MODE == HIST_PIX16) {
    const uint4 r = *reinterpret_cast<const uint4*>(base + t * a.ld_t + i * a.ld_p);
    const unsigned u[4] = {r.x, r.y, r.z, r.w};
    if (sizeof(T) == 2) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c) v[0][c] = __uint_as_float(c & 1 ? u[c / 2] & 0xffff0000u : u[c / 2] << 16);
    } else {
#pragma unroll
      for (int c = 0; c < MAXC; ++c) v[0][c] = c < 4 ? __uint_as_float(u[c & 3]) : 0.f;
    }
  } else {
    const T* q = base + t * a.ld_t + i * a.ld_p;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < a.C) v[0][c] = ld_elem(q + c * a.ld_c);
  }
}

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
  const int nb3 = a.nbins + 3, nout = a.C + a.speed;
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
    load_item<T, MODE>(a, t, i, v);
    t += dt;
    i += di;
    if (i >= a.ipf) { i -= a.ipf; ++t; }
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      float yu = 0.f, yv = 0.f;
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        if (c < a.C) {
          const float y = hist_affine(v[k][c], a.scale[c], a.offset[c]);
          atomicAdd(&hist_lds[c * nb3 + hist_bin(y, a.lo[c], a.inv_w[c], a.nbins)], 1u);
          acc[c].add(y);
          yu = c == a.su ? y : yu;
          yv = c == a.sv ? y : yv;
        }
      }
      if (a.speed) {
        const float s = hist_speed(yu, yv);
        atomicAdd(&hist_lds[a.C * nb3 + hist_bin(s, a.lo[a.C], a.inv_w[a.C], a.nbins)], 1u);
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
      acc[j].s1 += shfl_xor_d(acc[j].s1, m);
      acc[j].s2 += shfl_xor_d(acc[j].s2, m);
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
  if (!s || s->nbins < 1 || s->nbins > DG_HIST_MAX_BINS || C < 1 || C > MAXC) return false;
  const bool speed = s->speed_u >= 0 || s->speed_v >= 0;
  if (speed && (s->speed_u < 0 || s->speed_u >= C || s->speed_v < 0 || s->speed_v >= C)) return false;
  const int nout = C + (speed ? 1 : 0);
  for (int j = 0; j < nout; ++j)
    if (!(fabsf(s->lo[j]) <= FLT_MAX) || !(s->inv_w[j] > 0.f && s->inv_w[j] <= FLT_MAX)) return false;
  for (int c = 0; c < C; ++c)
    if (!(fabsf(s->scale[c]) <= FLT_MAX) || !(fabsf(s->offset[c]) <= FLT_MAX)) return false;
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
  const bool speed = s->speed_u >= 0;
  for (int64_t i = 0; i < n; ++i) {
    float yu = 0.f, yv = 0.f;
    for (int c = 0; c < C; ++c) {
      const float y = hist_affine(x[(int64_t)c * n + i], s->scale[c], s->offset[c]);
      bins[(int64_t)c * n + i] = hist_bin(y, s->lo[c], s->inv_w[c], s->nbins);
      if (c == s->speed_u) yu = y;
      if (c == s->speed_v) yv = y;
    }
    if (speed) bins[(int64_t)C * n + i] = hist_bin(hist_speed(yu, yv), s->lo[C], s->inv_w[C], s->nbins);
  }
  return DG_OK;
}

extern "C" int dg_hist(const dg_eof_fields* x, const dg_hist_spec* s, void* ws, int64_t* counts, double* moments, float* extrema,
                       void* stream) {
  if (!hist_fields_ok(x) || !spec_ok(s, x->C) || !ws || !counts || !moments || !extrema) return DG_ERR_BAD_SHAPE;
  if (x->dtype != DG_F32 && x->dtype != DG_BF16) return DG_ERR_BAD_DTYPE;
  const int mode = hist_mode(x);
  const int speed = s->speed_u >= 0 ? 1 : 0, nout = x->C + speed;
  HistArgs a;
  a.base = x->base; a.ld_t = x->ld_t; a.ld_c = x->ld_c; a.ld_p = x->ld_p;
  a.C = x->C; a.P = x->P; a.nbins = s->nbins; a.speed = speed; a.su = s->speed_u; a.sv = s->speed_v;
  a.ipf = mode == HIST_NCHW4 ? x->P / 4 : x->P;
  for (int j = 0; j < MAXO; ++j) {
    a.lo[j] = j < nout ? s->lo[j] : 0.f;
    a.inv_w[j] = j < nout ? s->inv_w[j] : 1.f;
  }
  for (int c = 0; c < MAXC; ++c) {
    a.scale[c] = c < x->C ? s->scale[c] : 1.f;
    a.offset[c] = c < x->C ? s->offset[c] : 0.f;
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
    int rc;
    if (x->dtype == DG_F32)
      rc = mode == HIST_NCHW4 ? launch<float, HIST_NCHW4>(a, grid, lds, st)
         : mode == HIST_PIX16 ? launch<float, HIST_PIX16>(a, grid, lds, st) : launch<float, HIST_ANY>(a, grid, lds, st);
    else
      rc = mode == HIST_NCHW4 ? launch<bf16_t, HIST_NCHW4>(a, grid, lds, st)
         : mode == HIST_PIX16 ? launch<bf16_t, HIST_PIX16>(a, grid, lds, st) : launch<bf16_t, HIST_ANY>(a, grid, lds, st);
    if (rc != DG_OK) return rc;
    hipLaunchKernelGGL(hist_finish_kernel, dim3(nout), dim3(HIST_THREADS), 0, st, (const double*)a.part_m, (const float*)a.part_e,
                       grid, x->C, moments, extrema);
  }
  return dg_check_launch();
}
