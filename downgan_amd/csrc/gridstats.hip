// Per-gridpoint statistics (include/downgan_hip.h "Per-gridpoint statistics") of one or two series of fields read through the
// EOF descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16), any T and P.  The reduction runs over t and keeps p: the
// opposite of hist_kernel, and bandwidth-bound like it.
//   gridstats_kernel<TA, MA, TB, MB, PAIRED>
//       A thread owns its pixels (MA = MB = HIST_NCHW4: four consecutive pixels, one 16 B / 8 B load per channel plane and
//       field; otherwise one pixel: HIST_PIX16 = one 16-byte load per field, HIST_ANY = one element per load), a wave's pixels
//       are contiguous.  It walks its slice of t, GS_UNROLL fields of both series loaded before the first is consumed, with the
//       running state of GS units in registers: 4 pixels x 1 output channel, or 1 pixel x 3 output channels (C = 2 + speed in
//       one pass over the input; wider specs walk the output channels in groups of that size and re-read the input per
//       group).  At the end it touches the accumulator rows once: pixel-contiguous, so the read-modify-write is coalesced.
//       One slice: += into the accumulators.  More: plain stores to the slice's rows of the workspace.
//   gridstats_finish_kernel
//       element-wise over the accumulator arrays: the slices added in slice order (fixed), += / min / max into the accumulators.
// No atomics, no LDS, no cross-lane traffic: every sum is a t-ordered chain of one thread, so two calls are bit-identical.
// The output values y come from hist_common.h, the code histogram.hip bins.
#include <float.h>
#include <math.h>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_UNROLL = 4;                          // fields in flight per series (2 with four pixels per thread and two series:
                                                      // 4 x 39 registers of state leave no room for more loads)
constexpr int GS_WAVES_PER_SIMD = 2;                  // the register budget: 256 VGPRs per thread
constexpr int GS_FINISH_GRID_MAX = 2048;
constexpr int GS_BLOCKS_FULL = 1024;                  // pixel blocks of 256 that fill the chip without a T-split
constexpr int GS_SLICE_MIN_T = 16;                    // fields per slice at least
constexpr int MAXO = DG_HIST_MAX_OUT, MAXK = DG_GRID_MAX_THR;

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef int i4_t __attribute__((ext_vector_type(4)));

struct GsArgs {
  HistSeries a, b;
  HistXform xf;
  int P, T, nout, nthr, slices, accumulate;
  float pivot[MAXO], thr[MAXO][MAXK];
  double* sums;               // the accumulators (one slice), or slice 0 of the workspace
  float* ext;
  int* cnt;
  long long slice_sums, slice_ext, slice_cnt;         // elements from one slice of the workspace to the next
};

// what one unit of state does with its output values
struct Unit : HistUnit {
  float thr[MAXK];
  double pivot;
};

struct Side {
  double s1, s2, s3, s4;
  float mn, mx;
  int n, e[MAXK];
  __device__ __forceinline__ void init() {
    s1 = s2 = s3 = s4 = 0.0; mn = INFINITY; mx = -INFINITY; n = 0;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) e[k] = 0;
  }
  // returns u = y - pivot (0 for an invalid y)
  __device__ __forceinline__ double add(float y, bool fin, const Unit& un) {
    const double u = fin ? (double)y - un.pivot : 0.0;
    const double u2 = u * u;
    s1 += u; s2 += u2; s3 += u2 * u; s4 += u2 * u2;
    n += fin ? 1 : 0;
    mn = fin ? fminf(mn, y) : mn;
    mx = fin ? fmaxf(mx, y) : mx;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) e[k] += y > un.thr[k] ? 1 : 0;   // unused thresholds are +inf: never exceeded
    return u;
  }
};

struct Pair {
  double d1, da, d2, x;
  int n;
  __device__ __forceinline__ void init() { d1 = da = d2 = x = 0.0; n = 0; }
  __device__ __forceinline__ void add(float ya, float yb, bool fa, bool fb, double ua, double ub) {
    const bool both = fa && fb;
    const double d = both ? (double)yb - (double)ya : 0.0;
    d1 += d; da += fabs(d); d2 += d * d;
    x += ua * ub;                                                    // u is 0 for an invalid value
    n += both ? 1 : 0;
  }
};

__device__ __forceinline__ void put(double* q, double v, bool acc) { *q = acc ? *q + v : v; }
__device__ __forceinline__ void put(int* q, int v, bool acc) { *q = acc ? *q + v : v; }
__device__ __forceinline__ void put_min(float* q, float v, bool acc) { *q = acc ? fminf(*q, v) : v; }
__device__ __forceinline__ void put_max(float* q, float v, bool acc) { *q = acc ? fmaxf(*q, v) : v; }
// four consecutive pixels of one row (the launcher checked the alignment of the rows)
__device__ __forceinline__ void put4(double* q, const double (&v)[4], bool acc) {
  d4_t o = {v[0], v[1], v[2], v[3]};
  if (acc) o += *reinterpret_cast<const d4_t*>(q);
  *reinterpret_cast<d4_t*>(q) = o;
}
__device__ __forceinline__ void put4(int* q, const int (&v)[4], bool acc) {
  i4_t o = {v[0], v[1], v[2], v[3]};
  if (acc) o += *reinterpret_cast<const i4_t*>(q);
  *reinterpret_cast<i4_t*>(q) = o;
}
__device__ __forceinline__ void put4_minmax(float* q, const float (&v)[4], bool acc, bool is_min) {
  f4_t o = {v[0], v[1], v[2], v[3]};
  if (acc) {
    const f4_t p = *reinterpret_cast<const f4_t*>(q);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = is_min ? fminf(p[k], o[k]) : fmaxf(p[k], o[k]);
  }
  *reinterpret_cast<f4_t*>(q) = o;
}

// one group of output channels over the fields [t0, t1) of this thread's pixels, then its rows of the accumulators
template <typename TA, int MA, typename TB, int MB, bool PAIRED, bool SPD, int UNITS>
__device__ __forceinline__ void gs_group(const GsArgs& g, const Unit (&un)[UNITS], long long i, long long t0, long long t1,
                                         double* sums, float* ext, int* cnt) {
  constexpr bool QUAD = MA == HIST_NCHW4;
  Side sa[UNITS], sb[UNITS];
  Pair pr[UNITS];
#pragma unroll
  for (int k = 0; k < UNITS; ++k) { sa[k].init(); sb[k].init(); pr[k].init(); }

  auto consume = [&](const HistRaw<MA, UNITS>& ra, const HistRaw<MB, UNITS>& rb) {
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      const float ya = hist_unit_value<TA, MA, UNITS, SPD>(ra, un[k], k);
      const bool fa = fabsf(ya) <= FLT_MAX;                          // false for NaN and +-inf
      const double ua = sa[k].add(ya, fa, un[k]);
      if (PAIRED) {
        const float yb = hist_unit_value<TB, MB, UNITS, SPD>(rb, un[k], k);
        const bool fb = fabsf(yb) <= FLT_MAX;
        const double ub = sb[k].add(yb, fb, un[k]);
        pr[k].add(ya, yb, fa, fb, ua, ub);
      }
    }
  };
  constexpr int U = QUAD && PAIRED ? GS_UNROLL / 2 : GS_UNROLL;
  long long t = t0;
  for (; t + U <= t1; t += U) {
    HistRaw<MA, UNITS> ra[U];
    HistRaw<MB, UNITS> rb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      hist_unit_load<TA, MA, UNITS, SPD>(g.a, t + u, i, un, ra[u]);
      if (PAIRED) hist_unit_load<TB, MB, UNITS, SPD>(g.b, t + u, i, un, rb[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) consume(ra[u], rb[u]);
  }
  for (; t < t1; ++t) {
    HistRaw<MA, UNITS> ra;
    HistRaw<MB, UNITS> rb;
    hist_unit_load<TA, MA, UNITS, SPD>(g.a, t, i, un, ra);
    if (PAIRED) hist_unit_load<TB, MB, UNITS, SPD>(g.b, t, i, un, rb);
    consume(ra, rb);
  }

  // rows of output channel j (the layout of the header), pixel fastest
  constexpr int NS = PAIRED ? 12 : 4, NE = PAIRED ? 4 : 2;
  const int NC = PAIRED ? 3 + 2 * g.nthr : 1 + g.nthr, e0 = PAIRED ? 3 : 1;
  const long long P = g.P;
  const bool acc = g.accumulate != 0;
  if constexpr (QUAD) {
    const int j = un[0].j;                                           // one output channel, four consecutive pixels
    const long long p = 4 * i;
    double* qs = sums + (long long)j * NS * P + p;
    float* qe = ext + (long long)j * NE * P + p;
    int* qc = cnt + (long long)j * NC * P + p;
#define GS_D4(row, expr) { const double v_[4] = {sa[0] expr, sa[1] expr, sa[2] expr, sa[3] expr}; put4(qs + (row) * P, v_, acc); }
#define GS_D4B(row, expr) { const double v_[4] = {sb[0] expr, sb[1] expr, sb[2] expr, sb[3] expr}; put4(qs + (row) * P, v_, acc); }
#define GS_D4P(row, expr) { const double v_[4] = {pr[0] expr, pr[1] expr, pr[2] expr, pr[3] expr}; put4(qs + (row) * P, v_, acc); }
    GS_D4(0, .s1) GS_D4(1, .s2) GS_D4(2, .s3) GS_D4(3, .s4)
    { const float v_[4] = {sa[0].mn, sa[1].mn, sa[2].mn, sa[3].mn}; put4_minmax(qe, v_, acc, true); }
    { const float v_[4] = {sa[0].mx, sa[1].mx, sa[2].mx, sa[3].mx}; put4_minmax(qe + P, v_, acc, false); }
    { const int v_[4] = {sa[0].n, sa[1].n, sa[2].n, sa[3].n}; put4(qc, v_, acc); }
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (k < g.nthr) { const int v_[4] = {sa[0].e[k], sa[1].e[k], sa[2].e[k], sa[3].e[k]}; put4(qc + (e0 + k) * P, v_, acc); }
    if (PAIRED) {
      GS_D4B(4, .s1) GS_D4B(5, .s2) GS_D4B(6, .s3) GS_D4B(7, .s4)
      GS_D4P(8, .d1) GS_D4P(9, .da) GS_D4P(10, .d2) GS_D4P(11, .x)
      { const float v_[4] = {sb[0].mn, sb[1].mn, sb[2].mn, sb[3].mn}; put4_minmax(qe + 2 * P, v_, acc, true); }
      { const float v_[4] = {sb[0].mx, sb[1].mx, sb[2].mx, sb[3].mx}; put4_minmax(qe + 3 * P, v_, acc, false); }
      { const int v_[4] = {sb[0].n, sb[1].n, sb[2].n, sb[3].n}; put4(qc + P, v_, acc); }
      { const int v_[4] = {pr[0].n, pr[1].n, pr[2].n, pr[3].n}; put4(qc + 2 * P, v_, acc); }
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k < g.nthr) {
          const int v_[4] = {sb[0].e[k], sb[1].e[k], sb[2].e[k], sb[3].e[k]};
          put4(qc + (e0 + g.nthr + k) * P, v_, acc);
        }
    }
#undef GS_D4
#undef GS_D4B
#undef GS_D4P
  } else {
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
      if (!un[u].on) continue;                                       // wave-uniform: nothing beyond the real channels
      const int j = un[u].j;
      double* qs = sums + (long long)j * NS * P + i;
      float* qe = ext + (long long)j * NE * P + i;
      int* qc = cnt + (long long)j * NC * P + i;
      put(qs, sa[u].s1, acc); put(qs + P, sa[u].s2, acc); put(qs + 2 * P, sa[u].s3, acc); put(qs + 3 * P, sa[u].s4, acc);
      put_min(qe, sa[u].mn, acc); put_max(qe + P, sa[u].mx, acc);
      put(qc, sa[u].n, acc);
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k < g.nthr) put(qc + (e0 + k) * P, sa[u].e[k], acc);
      if (PAIRED) {
        put(qs + 4 * P, sb[u].s1, acc); put(qs + 5 * P, sb[u].s2, acc); put(qs + 6 * P, sb[u].s3, acc); put(qs + 7 * P, sb[u].s4, acc);
        put(qs + 8 * P, pr[u].d1, acc); put(qs + 9 * P, pr[u].da, acc); put(qs + 10 * P, pr[u].d2, acc); put(qs + 11 * P, pr[u].x, acc);
        put_min(qe + 2 * P, sb[u].mn, acc); put_max(qe + 3 * P, sb[u].mx, acc);
        put(qc + P, sb[u].n, acc); put(qc + 2 * P, pr[u].n, acc);
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
          if (k < g.nthr) put(qc + (e0 + g.nthr + k) * P, sb[u].e[k], acc);
      }
    }
  }
}

template <typename TA, int MA, typename TB, int MB, bool PAIRED>
__global__ __launch_bounds__(GS_THREADS, GS_WAVES_PER_SIMD) void gridstats_kernel(GsArgs g) {
  constexpr bool QUAD = MA == HIST_NCHW4;
  static_assert(!PAIRED || QUAD == (MB == HIST_NCHW4), "both series share the pixel ownership");
  constexpr int UNITS = QUAD ? 4 : 3;
  const long long i = (long long)blockIdx.x * GS_THREADS + threadIdx.x;
  if (i >= (QUAD ? g.P / 4 : g.P)) return;
  const long long slice = blockIdx.y;
  const long long t0 = slice * g.T / g.slices, t1 = (slice + 1) * g.T / g.slices;
  double* sums = g.sums + slice * g.slice_sums;
  float* ext = g.ext + slice * g.slice_ext;
  int* cnt = g.cnt + slice * g.slice_cnt;
  const int ngroups = QUAD ? g.nout : (g.nout + UNITS - 1) / UNITS;
  for (int grp = 0; grp < ngroups; ++grp) {
    Unit un[UNITS];
    bool any_speed = false;
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      const int j = QUAD ? grp : grp * UNITS + k;
      Unit& w = un[k];
      w.on = j < g.nout;
      w.j = w.on ? j : 0;
      w.spd = g.xf.speed && w.j == g.xf.C;
      any_speed |= w.spd;
      w.c1 = w.spd ? g.xf.su : w.j;
      w.c2 = w.spd ? g.xf.sv : w.j;
      w.sc1 = g.xf.scale[w.c1]; w.of1 = g.xf.offset[w.c1];
      w.sc2 = g.xf.scale[w.c2]; w.of2 = g.xf.offset[w.c2];
      w.pivot = (double)g.pivot[w.j];
#pragma unroll
      for (int q = 0; q < MAXK; ++q) w.thr[q] = q < g.nthr ? g.thr[w.j][q] : INFINITY;
    }
    if (any_speed)
      gs_group<TA, MA, TB, MB, PAIRED, true, UNITS>(g, un, i, t0, t1, sums, ext, cnt);
    else
      gs_group<TA, MA, TB, MB, PAIRED, false, UNITS>(g, un, i, t0, t1, sums, ext, cnt);
  }
}

// acc[i] (+=, min, max) the slices 0 .. S-1 of ws[s][i], in slice order
__global__ __launch_bounds__(GS_THREADS) void gridstats_finish_kernel(const double* ws_s, const float* ws_e, const int* ws_c, int S,
                                                                      long long n_s, long long n_e, long long n_c, long long P,
                                                                      double* sums, float* ext, int* cnt) {
  const long long stride = (long long)gridDim.x * GS_THREADS, i0 = (long long)blockIdx.x * GS_THREADS + threadIdx.x;
  for (long long i = i0; i < n_s; i += stride) {
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += ws_s[s * n_s + i];
    sums[i] += v;
  }
  for (long long i = i0; i < n_e; i += stride) {
    const bool is_min = ((i / P) & 1) == 0;                         // rows alternate min, max
    float v = ext[i];
    for (int s = 0; s < S; ++s) v = is_min ? fminf(v, ws_e[s * n_e + i]) : fmaxf(v, ws_e[s * n_e + i]);
    ext[i] = v;
  }
  for (long long i = i0; i < n_c; i += stride) {
    int v = 0;
    for (int s = 0; s < S; ++s) v += ws_c[s * n_c + i];
    cnt[i] += v;
  }
}

bool spec_ok(const dg_grid_spec* s, int C) {
  if (!s || s->nthr < 0 || s->nthr > MAXK || !hist_xform_ok(s, C)) return false;
  const int nout = hist_nout(s, C);
  for (int j = 0; j < nout; ++j)
    if (!hist_finite(s->pivot[j])) return false;
  return hist_thr_ok(s->thr, nout, s->nthr);
}

int slices_of(int T, int P) {
  if (T < 1 || P < 1) return 0;
  const int nb = (int)(((long long)P + 255) / 256);
  if (nb >= GS_BLOCKS_FULL) return 1;
  const int want = (GS_BLOCKS_FULL + nb - 1) / nb, cap = T / GS_SLICE_MIN_T;
  const int s = want < cap ? want : cap;
  return s < 1 ? 1 : s;
}

struct Layout {
  int nout, NS, NE, NC, S;
  size_t n_s, n_e, n_c;       // elements of one slice = of the accumulators
  size_t off_e, off_c, bytes; // workspace sections
};

Layout layout_of(const dg_eof_fields* a, bool paired, const dg_grid_spec* s) {
  Layout l;
  l.nout = hist_nout(s, a->C);
  l.NS = paired ? 12 : 4;
  l.NE = paired ? 4 : 2;
  l.NC = paired ? 3 + 2 * s->nthr : 1 + s->nthr;
  l.S = slices_of(a->T, a->P);
  const size_t np = (size_t)l.nout * (size_t)a->P;
  l.n_s = np * l.NS; l.n_e = np * l.NE; l.n_c = np * l.NC;
  if (l.S == 1) {
    l.off_e = l.off_c = 0;
    l.bytes = 256;
  } else {
    l.off_e = hist_round256(l.S * l.n_s * sizeof(double));
    l.off_c = l.off_e + hist_round256(l.S * l.n_e * sizeof(float));
    l.bytes = l.off_c + hist_round256(l.S * l.n_c * sizeof(int));
  }
  return l;
}

// a series read by a one-pixel-per-thread kernel: HIST_NCHW4 planes are read element by element
int single_mode(const dg_eof_fields* x) {
  const int m = hist_mode(x);
  return m == HIST_NCHW4 ? HIST_ANY : m;
}

bool aligned(const void* p, size_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

template <typename TA, int MA, typename TB, int MB, bool PAIRED>
void launch(const GsArgs& g, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((gridstats_kernel<TA, MA, TB, MB, PAIRED>), grid, dim3(GS_THREADS), 0, st, g);
}

template <typename TA, int MA, bool PAIRED>
void launch_b(int mb, bool b_bf16, const GsArgs& g, dim3 grid, hipStream_t st) {
  if constexpr (!PAIRED) {
    launch<TA, MA, TA, MA, false>(g, grid, st);
  } else if constexpr (MA == HIST_NCHW4) {
    if (b_bf16) launch<TA, MA, bf16_t, HIST_NCHW4, true>(g, grid, st);
    else launch<TA, MA, float, HIST_NCHW4, true>(g, grid, st);
  } else {
    if (mb == HIST_PIX16) {
      if (b_bf16) launch<TA, MA, bf16_t, HIST_PIX16, true>(g, grid, st);
      else launch<TA, MA, float, HIST_PIX16, true>(g, grid, st);
    } else {
      if (b_bf16) launch<TA, MA, bf16_t, HIST_ANY, true>(g, grid, st);
      else launch<TA, MA, float, HIST_ANY, true>(g, grid, st);
    }
  }
}

template <bool PAIRED>
void launch_a(int ma, bool a_bf16, int mb, bool b_bf16, const GsArgs& g, dim3 grid, hipStream_t st) {
  if (ma == HIST_NCHW4) {
    if (a_bf16) launch_b<bf16_t, HIST_NCHW4, PAIRED>(mb, b_bf16, g, grid, st);
    else launch_b<float, HIST_NCHW4, PAIRED>(mb, b_bf16, g, grid, st);
  } else if (ma == HIST_PIX16) {
    if (a_bf16) launch_b<bf16_t, HIST_PIX16, PAIRED>(mb, b_bf16, g, grid, st);
    else launch_b<float, HIST_PIX16, PAIRED>(mb, b_bf16, g, grid, st);
  } else {
    if (a_bf16) launch_b<bf16_t, HIST_ANY, PAIRED>(mb, b_bf16, g, grid, st);
    else launch_b<float, HIST_ANY, PAIRED>(mb, b_bf16, g, grid, st);
  }
}

}  // namespace

extern "C" int dg_gridstats_slices(int T, int P) { return slices_of(T, P); }

extern "C" size_t dg_gridstats_ws_bytes(const dg_eof_fields* a, int paired, const dg_grid_spec* s) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C)) return 0;
  return layout_of(a, paired != 0, s).bytes;
}

extern "C" int dg_gridstats(const dg_eof_fields* a, const dg_eof_fields* b, const dg_grid_spec* s, void* ws, double* sums,
                            float* extrema, int32_t* counts, void* stream) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C) || !sums || !extrema || !counts) return DG_ERR_BAD_SHAPE;
  const bool paired = b != nullptr;
  if (paired && (!hist_fields_ok(b) || b->T != a->T || b->C != a->C || b->P != a->P)) return DG_ERR_BAD_SHAPE;
  const Layout l = layout_of(a, paired, s);
  if (l.S > 1 && !ws) return DG_ERR_BAD_SHAPE;
  if ((a->dtype != DG_F32 && a->dtype != DG_BF16) || (paired && b->dtype != DG_F32 && b->dtype != DG_BF16)) return DG_ERR_BAD_DTYPE;

  GsArgs g;
  g.a = hist_series(a);
  g.b = paired ? hist_series(b) : g.a;
  g.xf = hist_xform(s, a->C);
  g.P = a->P; g.T = a->T; g.nout = l.nout;
  g.nthr = s->nthr; g.slices = l.S; g.accumulate = l.S == 1 ? 1 : 0;
  for (int j = 0; j < MAXO; ++j) g.pivot[j] = j < l.nout ? s->pivot[j] : 0.f;
  hist_thr_pad(s->thr, l.nout, s->nthr, g.thr);
  char* w = reinterpret_cast<char*>(ws);
  if (l.S == 1) {
    g.sums = sums; g.ext = extrema; g.cnt = counts;
    g.slice_sums = g.slice_ext = g.slice_cnt = 0;
  } else {
    g.sums = reinterpret_cast<double*>(w);
    g.ext = reinterpret_cast<float*>(w + l.off_e);
    g.cnt = reinterpret_cast<int*>(w + l.off_c);
    g.slice_sums = (long long)l.n_s; g.slice_ext = (long long)l.n_e; g.slice_cnt = (long long)l.n_c;
  }
  // four pixels per thread when both series are NCHW planes that allow it and the rows the kernel writes are aligned for
  // 32- / 16-byte accesses (P % 4 == 0 then keeps every row and slice aligned); one pixel per thread otherwise
  const bool quad = hist_mode(a) == HIST_NCHW4 && (!paired || hist_mode(b) == HIST_NCHW4) && aligned(g.sums, 32) &&
                    aligned(g.ext, 16) && aligned(g.cnt, 16);
  const int ma = quad ? HIST_NCHW4 : single_mode(a), mb = !paired ? ma : quad ? HIST_NCHW4 : single_mode(b);
  const long long ipf = quad ? a->P / 4 : a->P;
  const dim3 grid((unsigned)((ipf + GS_THREADS - 1) / GS_THREADS), (unsigned)l.S);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (paired) launch_a<true>(ma, a->dtype == DG_BF16, mb, b->dtype == DG_BF16, g, grid, st);
  else launch_a<false>(ma, a->dtype == DG_BF16, ma, a->dtype == DG_BF16, g, grid, st);
  if (l.S > 1) {
    const size_t nmax = l.n_s > l.n_c ? l.n_s : l.n_c;
    size_t fg = (nmax + GS_THREADS - 1) / GS_THREADS;
    fg = fg > (size_t)GS_FINISH_GRID_MAX ? GS_FINISH_GRID_MAX : fg;
    hipLaunchKernelGGL(gridstats_finish_kernel, dim3((unsigned)fg), dim3(GS_THREADS), 0, st, (const double*)g.sums, (const float*)g.ext,
                       (const int*)g.cnt, l.S, (long long)l.n_s, (long long)l.n_e, (long long)l.n_c, (long long)a->P, sums, extrema,
                       counts);
  }
  return dg_check_launch();
}
