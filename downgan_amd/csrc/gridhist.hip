// Per-gridpoint histograms (include/downgan_hip.h "Per-gridpoint histograms") of one or two series of fields read through the
// EOF descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16), any T and P: the table int32 [nout][S][nbins + 3][P], and the
// scan that turns it into quantile ranks and the integer W1 / KS sums.
//   gridhist_kernel<TA, MA, TB, MB, PAIRED>
//       The pixel ownership of gridstats_kernel: a thread owns four consecutive pixels (MA = MB = HIST_NCHW4: one 16 B / 8 B
//       load per channel plane and field) or one pixel (HIST_PIX16 = one 16-byte load per field, HIST_ANY = one element per
//       load); a wave's pixels are contiguous, so lanes that fall into the same row add into one segment of that row's plane.
//       blockIdx.y cuts the fields into slices.  A thread walks its slice in t order, GH_UNROLL fields of both series loaded
//       before the first is consumed, with (row, run length) per unit and side in registers: 4 pixels x 1 output channel, or
//       1 pixel x 3 output channels (wider specs walk the output channels in groups and re-read the input per group).  A run of
//       equal rows is added once, when it ends, with a no-return 32-bit integer atomic at agent scope.
//   gridhist_scan_kernel<NPX, QM>
//       one lane per NPX pixels (4: 16-byte loads of every row) of one output channel: a first walk over the rows of both sides
//       for the finite totals, the Q targets per side into registers, a second walk with the cumulative counts that stores each
//       rank triple in the row where its target is reached and sums the two distances.  No atomics, no LDS.
// The output values y and their rows come from hist_common.h, the code histogram.hip bins.  Integer adds commute, so the table
// is exact and two calls are bit-identical.
#include <float.h>
#include <math.h>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int GH_THREADS = 256;
constexpr int GH_UNROLL = 4;                          // fields in flight per series
constexpr int GH_BLOCKS_FULL = 1024;                  // workgroups that fill the chip without cutting the fields
constexpr int GH_SLICE_MIN_T = 8;                     // fields per slice at least: runs of equal rows stay worth combining
constexpr int MAXO = DG_HIST_MAX_OUT, MAXQ = DG_GRIDHIST_MAX_Q;

struct GhArgs {
  HistSeries a, b;
  int P, T, nout, nbins;
  HistXform xf;
  float lo[MAXO], inv_w[MAXO];
  int slices;
  int* counts;
};

// how one unit of state bins its output values
struct Unit : HistUnit {
  float lo, inv_w;
};

// the open run of one unit and side: `run` consecutive fields fell in `row` of the plane `base` (this thread's pixel of it)
struct Run {
  int* base;
  int row, run;
  __device__ __forceinline__ void init(int* b) { base = b; row = 0; run = 0; }
  __device__ __forceinline__ void flush(long long P) {
    if (run > 0) __hip_atomic_fetch_add(base + (long long)row * P, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void push(int r, long long P) {
    if (r != row) { flush(P); row = r; run = 0; }
    ++run;
  }
};

// the row of unit k
template <typename T, int MODE, int UNITS, bool SPD>
__device__ __forceinline__ int gh_row(const HistRaw<MODE, UNITS>& r, const Unit& un, int k, int nbins) {
  return hist_bin(hist_unit_value<T, MODE, UNITS, SPD>(r, un, k), un.lo, un.inv_w, nbins);
}

// one group of output channels over the fields [t0, t1) of this thread's pixels
template <typename TA, int MA, typename TB, int MB, bool PAIRED, bool SPD, int UNITS>
__device__ __forceinline__ void gh_group(const GhArgs& g, const Unit (&un)[UNITS], long long i, long long t0, long long t1) {
  constexpr bool QUAD = MA == HIST_NCHW4;
  constexpr int S = PAIRED ? 2 : 1;
  const long long P = g.P, plane = (long long)(g.nbins + 3) * P;
  Run ra_[UNITS], rb_[UNITS];
#pragma unroll
  for (int k = 0; k < UNITS; ++k) {
    const long long p = QUAD ? 4 * i + k : i;                        // QUAD: one output channel, four consecutive pixels
    int* q = g.counts + (long long)un[k].j * S * plane + p;
    ra_[k].init(q);
    rb_[k].init(q + plane);
  }
  auto consume = [&](const HistRaw<MA, UNITS>& a, const HistRaw<MB, UNITS>& b) {
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      if (!un[k].on) continue;                                       // wave-uniform: nothing beyond the real channels
      ra_[k].push(gh_row<TA, MA, UNITS, SPD>(a, un[k], k, g.nbins), P);
      if (PAIRED) rb_[k].push(gh_row<TB, MB, UNITS, SPD>(b, un[k], k, g.nbins), P);
    }
  };
  constexpr int U = QUAD && PAIRED ? GH_UNROLL / 2 : GH_UNROLL;
  long long t = t0;
  for (; t + U <= t1; t += U) {
    HistRaw<MA, UNITS> a[U];
    HistRaw<MB, UNITS> b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      hist_unit_load<TA, MA, UNITS, SPD>(g.a, t + u, i, un, a[u]);
      if (PAIRED) hist_unit_load<TB, MB, UNITS, SPD>(g.b, t + u, i, un, b[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) consume(a[u], b[u]);
  }
  for (; t < t1; ++t) {
    HistRaw<MA, UNITS> a;
    HistRaw<MB, UNITS> b;
    hist_unit_load<TA, MA, UNITS, SPD>(g.a, t, i, un, a);
    if (PAIRED) hist_unit_load<TB, MB, UNITS, SPD>(g.b, t, i, un, b);
    consume(a, b);
  }
#pragma unroll
  for (int k = 0; k < UNITS; ++k) {
    if (!un[k].on) continue;
    ra_[k].flush(P);
    if (PAIRED) rb_[k].flush(P);
  }
}

template <typename TA, int MA, typename TB, int MB, bool PAIRED>
__global__ __launch_bounds__(GH_THREADS) void gridhist_kernel(GhArgs g) {
  constexpr bool QUAD = MA == HIST_NCHW4;
  static_assert(!PAIRED || QUAD == (MB == HIST_NCHW4), "both series share the pixel ownership");
  constexpr int UNITS = QUAD ? 4 : 3;
  const long long i = (long long)blockIdx.x * GH_THREADS + threadIdx.x;
  if (i >= (QUAD ? g.P / 4 : g.P)) return;
  const long long slice = blockIdx.y;
  const long long t0 = slice * g.T / g.slices, t1 = (slice + 1) * g.T / g.slices;
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
      w.lo = g.lo[w.j]; w.inv_w = g.inv_w[w.j];
    }
    if (any_speed)
      gh_group<TA, MA, TB, MB, PAIRED, true, UNITS>(g, un, i, t0, t1);
    else
      gh_group<TA, MA, TB, MB, PAIRED, false, UNITS>(g, un, i, t0, t1);
  }
}

struct ScanQ {
  double q[MAXQ];
  int Q;
};

// k = (int64)ceil(fp64(q * fp64(n))): 1 <= k <= n < 2^31 for n >= 1 and 0 < q < 1, 0 for n = 0 (host and device)
__host__ __device__ inline int scan_target(double q, int n) {
  const double m = q * (double)n;
  return (int)(long long)ceil(m);
}
__host__ __device__ inline long long scan_absdiff(int A, int nb, int B, int na) {
  const long long d = (long long)A * nb - (long long)B * na;
  return d < 0 ? -d : d;
}

template <int NPX> struct Row { int v[NPX]; };
template <int NPX>
__device__ __forceinline__ Row<NPX> scan_load(const int* q) {
  Row<NPX> r;
  if constexpr (NPX == 4) {
    const int4 t = *reinterpret_cast<const int4*>(q);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *q;
  }
  return r;
}

// QM: the targets a lane keeps in registers (4 or MAXQ levels: the common three-level call runs at a quarter of the registers)
template <int NPX, int QM>
__global__ __launch_bounds__(GH_THREADS) void gridhist_scan_kernel(const int* counts, int S, int nbins, long long P, ScanQ qs,
                                                                   int* ranks, long long* dist) {
  const long long i = (long long)blockIdx.x * GH_THREADS + threadIdx.x;
  if (i >= P / NPX) return;
  const long long p0 = i * NPX, j = blockIdx.y;
  const int nb3 = nbins + 3, Q = qs.Q;
  const bool two = S == 2;
  const int* ca = counts + j * S * nb3 * P + p0;
  const int* cb = two ? ca + nb3 * P : ca;
  int na[NPX], nb[NPX];
#pragma unroll
  for (int k = 0; k < NPX; ++k) na[k] = nb[k] = 0;
  for (int r = 0; r < nbins + 2; ++r) {
    const Row<NPX> a = scan_load<NPX>(ca + r * P);
#pragma unroll
    for (int k = 0; k < NPX; ++k) na[k] += a.v[k];
    if (two) {
      const Row<NPX> b = scan_load<NPX>(cb + r * P);
#pragma unroll
      for (int k = 0; k < NPX; ++k) nb[k] += b.v[k];
    }
  }
  int ka[NPX][QM], kb[NPX][QM];
  int* ra = ranks + j * S * Q * 3 * P + p0;                          // [q][3][P] of side a; side b follows
  int* rb = ra + (long long)Q * 3 * P;
#pragma unroll
  for (int q = 0; q < QM; ++q) {
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      ka[k][q] = q < Q ? scan_target(qs.q[q], na[k]) : 0;
      kb[k][q] = q < Q && two ? scan_target(qs.q[q], nb[k]) : 0;
    }
    if (q < Q) {
#pragma unroll
      for (int k = 0; k < NPX; ++k) {
        if (na[k] == 0) { ra[(q * 3) * P + k] = -1; ra[(q * 3 + 1) * P + k] = 0; ra[(q * 3 + 2) * P + k] = 0; }
        if (two && nb[k] == 0) { rb[(q * 3) * P + k] = -1; rb[(q * 3 + 1) * P + k] = 0; rb[(q * 3 + 2) * P + k] = 0; }
      }
    }
  }
  int A[NPX], B[NPX];
  long long d0[NPX], d1[NPX];
#pragma unroll
  for (int k = 0; k < NPX; ++k) { A[k] = B[k] = 0; d0[k] = d1[k] = 0; }
  for (int r = 0; r < nbins + 2; ++r) {
    const Row<NPX> a = scan_load<NPX>(ca + r * P);
    Row<NPX> b = a;
    if (two) b = scan_load<NPX>(cb + r * P);
    const long long gw = r == 0 || r == nbins ? 1 : r < nbins ? 2 : 0;    // the weight of row r in the W1 sum
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      const int pa = A[k], pb = B[k];
      A[k] += a.v[k];
      B[k] += b.v[k];
#pragma unroll
      for (int q = 0; q < QM; ++q) {
        if (q < Q) {
          // the cumulative count is monotone and k >= 1: exactly one row has below < k <= through (none when n = 0: k = 0)
          if (pa < ka[k][q] && A[k] >= ka[k][q]) { ra[(q * 3) * P + k] = r; ra[(q * 3 + 1) * P + k] = pa; ra[(q * 3 + 2) * P + k] = a.v[k]; }
          if (two && pb < kb[k][q] && B[k] >= kb[k][q]) { rb[(q * 3) * P + k] = r; rb[(q * 3 + 1) * P + k] = pb; rb[(q * 3 + 2) * P + k] = b.v[k]; }
        }
      }
      if (two) {
        const long long d = scan_absdiff(A[k], nb[k], B[k], na[k]);
        d0[k] += gw * d;
        d1[k] = d > d1[k] ? d : d1[k];
      }
    }
  }
  if (two) {
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      const bool none = na[k] == 0 || nb[k] == 0;
      dist[(j * 2) * P + p0 + k] = none ? -1 : d0[k];
      dist[(j * 2 + 1) * P + p0 + k] = none ? -1 : d1[k];
    }
  }
}

bool spec_ok(const dg_hist_spec* s, int C) {
  if (!s || s->nbins < 1 || s->nbins > DG_GRIDHIST_MAX_BINS || !hist_xform_ok(s, C)) return false;
  for (int j = 0; j < hist_nout(s, C); ++j)
    if (!hist_finite(s->lo[j]) || !(s->inv_w[j] > 0.f && s->inv_w[j] <= FLT_MAX)) return false;
  return true;
}

bool scan_ok(const void* counts, int nout, int S, int nbins, int P, const double* q, int Q, const void* ranks, const void* dist) {
  if (!counts || !ranks || !q || nout < 1 || nout > MAXO || (S != 1 && S != 2) || nbins < 1 || nbins > DG_GRIDHIST_MAX_BINS || P < 1 ||
      Q < 1 || Q > MAXQ || (S == 2 && !dist))
    return false;
  for (int k = 0; k < Q; ++k)
    if (!(q[k] > 0.0 && q[k] < 1.0)) return false;                   // false for NaN
  return true;
}

// fields per workgroup column: one slice when the pixels alone fill the chip, else enough slices to, of GH_SLICE_MIN_T fields
int slices_of(int T, long long items) {
  const long long nb = (items + GH_THREADS - 1) / GH_THREADS;
  if (nb >= GH_BLOCKS_FULL) return 1;
  const long long want = (GH_BLOCKS_FULL + nb - 1) / nb, cap = T / GH_SLICE_MIN_T;
  const long long s = want < cap ? want : cap;
  return (int)(s < 1 ? 1 : s);
}

// a series read by a one-pixel-per-thread kernel: HIST_NCHW4 planes are read element by element
int single_mode(const dg_eof_fields* x) {
  const int m = hist_mode(x);
  return m == HIST_NCHW4 ? HIST_ANY : m;
}

template <typename TA, int MA, typename TB, int MB, bool PAIRED>
void launch(const GhArgs& g, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((gridhist_kernel<TA, MA, TB, MB, PAIRED>), grid, dim3(GH_THREADS), 0, st, g);
}

template <typename TA, int MA, bool PAIRED>
void launch_b(int mb, bool b_bf16, const GhArgs& g, dim3 grid, hipStream_t st) {
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
void launch_a(int ma, bool a_bf16, int mb, bool b_bf16, const GhArgs& g, dim3 grid, hipStream_t st) {
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

extern "C" size_t dg_gridhist_ws_bytes(const dg_eof_fields* a, int paired, const dg_hist_spec* s) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C)) return 0;
  return 256;                                                        // no partial state: the slices add into the table itself
}

extern "C" int dg_gridhist(const dg_eof_fields* a, const dg_eof_fields* b, const dg_hist_spec* s, void* ws, int32_t* counts,
                           void* stream) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C) || !counts) return DG_ERR_BAD_SHAPE;
  const bool paired = b != nullptr;
  if (paired && (!hist_fields_ok(b) || b->T != a->T || b->C != a->C || b->P != a->P)) return DG_ERR_BAD_SHAPE;
  if ((a->dtype != DG_F32 && a->dtype != DG_BF16) || (paired && b->dtype != DG_F32 && b->dtype != DG_BF16)) return DG_ERR_BAD_DTYPE;

  GhArgs g;
  g.a = hist_series(a);
  g.b = paired ? hist_series(b) : g.a;
  g.xf = hist_xform(s, a->C);
  g.P = a->P; g.T = a->T; g.nout = hist_nout(s, a->C); g.nbins = s->nbins;
  for (int j = 0; j < MAXO; ++j) {
    g.lo[j] = j < g.nout ? s->lo[j] : 0.f;
    g.inv_w[j] = j < g.nout ? s->inv_w[j] : 1.f;
  }
  g.counts = counts;
  // four pixels per thread when both series are NCHW planes that allow it; one pixel per thread otherwise
  const bool quad = hist_mode(a) == HIST_NCHW4 && (!paired || hist_mode(b) == HIST_NCHW4);
  const int ma = quad ? HIST_NCHW4 : single_mode(a), mb = !paired ? ma : quad ? HIST_NCHW4 : single_mode(b);
  const long long ipf = quad ? a->P / 4 : a->P;
  g.slices = slices_of(a->T, ipf);
  const dim3 grid((unsigned)((ipf + GH_THREADS - 1) / GH_THREADS), (unsigned)g.slices);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (paired) launch_a<true>(ma, a->dtype == DG_BF16, mb, b->dtype == DG_BF16, g, grid, st);
  else launch_a<false>(ma, a->dtype == DG_BF16, ma, a->dtype == DG_BF16, g, grid, st);
  return dg_check_launch();
}

extern "C" int dg_gridhist_scan(const int32_t* counts, int nout, int S, int nbins, int P, const double* q, int Q, int32_t* ranks,
                                int64_t* dist, void* stream) {
  if (!scan_ok(counts, nout, S, nbins, P, q, Q, ranks, dist)) return DG_ERR_BAD_SHAPE;
  ScanQ qs;
  qs.Q = Q;
  for (int k = 0; k < MAXQ; ++k) qs.q[k] = k < Q ? q[k] : 0.5;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  long long* d = reinterpret_cast<long long*>(dist);
  // four pixels per lane when every row of the table is aligned for 16-byte loads
  const bool quad = P % 4 == 0 && reinterpret_cast<uintptr_t>(counts) % 16 == 0;
  const long long items = quad ? P / 4 : P;
  const dim3 grid((unsigned)((items + GH_THREADS - 1) / GH_THREADS), (unsigned)nout);
  const bool few = Q <= 4;
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(GH_THREADS), 0, st, counts, S, nbins, (long long)P, qs, ranks, d); };
  if (quad) { if (few) go(gridhist_scan_kernel<4, 4>); else go(gridhist_scan_kernel<4, MAXQ>); }
  else { if (few) go(gridhist_scan_kernel<1, 4>); else go(gridhist_scan_kernel<1, MAXQ>); }
  return dg_check_launch();
}

extern "C" int dg_gridhist_host(const dg_hist_spec* s, const float* xa, const float* xb, int C, int T, int P, int32_t* counts) {
  if (!spec_ok(s, C) || T < 1 || P < 1 || !xa || !counts) return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C), S = xb ? 2 : 1, nb3 = s->nbins + 3;
  for (int side = 0; side < S; ++side) {
    const float* x = side ? xb : xa;
    for (int64_t t = 0; t < T; ++t)
      for (int64_t p = 0; p < P; ++p)
        for (int j = 0; j < nout; ++j) {
          const int r = hist_bin(hist_host_value(s, x + t * C * P, C, (size_t)P, (size_t)p, j), s->lo[j], s->inv_w[j], s->nbins);
          counts[(((int64_t)j * S + side) * nb3 + r) * P + p] += 1;
        }
  }
  return DG_OK;
}

extern "C" int dg_gridhist_scan_host(const int32_t* counts, int nout, int S, int nbins, int P, const double* q, int Q,
                                     int32_t* ranks, int64_t* dist) {
  if (!scan_ok(counts, nout, S, nbins, P, q, Q, ranks, dist)) return DG_ERR_BAD_SHAPE;
  const int64_t nb3 = nbins + 3, Pl = P;
  for (int64_t j = 0; j < nout; ++j)
    for (int64_t p = 0; p < Pl; ++p) {
      int n[2] = {0, 0};
      for (int s = 0; s < S; ++s) {
        const int32_t* c = counts + (j * S + s) * nb3 * Pl + p;
        for (int r = 0; r < nbins + 2; ++r) n[s] += c[r * Pl];
        for (int k = 0; k < Q; ++k) {
          int32_t* o = ranks + ((j * S + s) * Q + k) * 3 * Pl + p;
          o[0] = -1; o[Pl] = 0; o[2 * Pl] = 0;
          const int target = scan_target(q[k], n[s]);
          int cum = 0;
          for (int r = 0; r < nbins + 2 && n[s] > 0; ++r) {
            const int v = c[r * Pl];
            if (cum + v >= target) { o[0] = r; o[Pl] = cum; o[2 * Pl] = v; break; }
            cum += v;
          }
        }
      }
      if (S == 2) {
        const int32_t *ca = counts + (j * 2) * nb3 * Pl + p, *cb = ca + nb3 * Pl;
        int A = 0, B = 0;
        long long d0 = 0, d1 = 0;
        for (int r = 0; r < nbins + 2; ++r) {
          A += ca[r * Pl];
          B += cb[r * Pl];
          const long long d = scan_absdiff(A, n[1], B, n[0]);
          if (r <= nbins) d0 += (r == 0 || r == nbins ? 1 : 2) * d;
          d1 = d > d1 ? d : d1;
        }
        const bool none = n[0] == 0 || n[1] == 0;
        dist[(j * 2) * Pl + p] = none ? -1 : d0;
        dist[(j * 2 + 1) * Pl + p] = none ? -1 : d1;
      }
    }
  return DG_OK;
}
