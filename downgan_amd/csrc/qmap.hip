// Empirical quantile mapping (include/downgan_hip.h "Empirical quantile mapping"): the per-gridpoint bias correction
// y' = F_real^-1(F_gen(y)) from a paired dg_gridhist table.
//   qmap_fit_kernel<NPX>
//       the pixel ownership of gridhist_scan_kernel: one lane per NPX pixels (4: 16-byte loads of the generated rows and 16-byte
//       stores of the nodes) of one output channel.  A first walk over the rows of both sides for the finite totals, then one merge
//       walk over the bin edges k: the cumulative generated count G_k is looked up in the real cumulative counts, and the two
//       pointers into the real rows (s: the first B_s n_g >= G_k n_r; h: the last B_h n_g <= G_k n_r) only advance, each real
//       row read once per pointer.  No per-lane arrays, no LDS, no atomics.
//   qmap_apply_kernel<T, MODE>
//       a workgroup of QA_WAVES waves owns QA_PX = 64 consecutive pixels: per output channel it stages their transfer functions in
//       LDS as [node][pixel] (row loads coalesced; ds_read_b32 serves a wave in two groups of 32 lanes over 32 banks, and a lane
//       reading any node of its own pixel hits bank pixel mod 32, distinct within its group, so the gather is conflict-free
//       whatever rows the lanes fall in), then wave w streams the fields t0 + w, t0 + w + QA_WAVES, .. of the slice blockIdx.y,
//       QA_UNROLL fields' loads in flight: bin, two LDS reads, three flops, one coalesced store.
// The output values y come from hist_common.h, the code gridhist.hip bins; every step after them is integer arithmetic or one
// correctly rounded operation with contraction off (the qmap_* rules below, shared with the host references), so device and host
// agree bit for bit and two calls are bit-identical.
#include <float.h>
#include <math.h>

#include <vector>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int QF_THREADS = 256;
constexpr int QA_PX = 64;                             // pixels per workgroup: one wave's width, two lane groups of 32 banks
constexpr int QA_WAVES = 4;
constexpr int QA_THREADS = QA_PX * QA_WAVES;
constexpr int QA_UNROLL = 4;                          // fields in flight per wave
constexpr int QA_BLOCKS_FULL = 2048;                  // workgroups that fill the chip without cutting the fields
constexpr int QA_SLICE_MIN_T = 2 * QA_WAVES;          // fields per slice at least: the staged nodes are used more than once per wave
constexpr int MAXO = DG_HIST_MAX_OUT;

// ---- the arithmetic rules: each line is one correctly rounded operation ---------------------------------------------------------
// plo of an interior target: fp64(s - 1) + fp64(num) / fp64(den), num = X - B'_{s-1}, den = b[s] n_g (both below 2^52: exact)
__host__ __device__ inline double qmap_plo(int s, long long num, long long den) {
#pragma clang fp contract(off)
  const double frac = (double)num / (double)den;
  return (double)(s - 1) + frac;
}
__host__ __device__ inline double qmap_clamp(int k, double plo, double phi) {
  const double a = (double)k > plo ? (double)k : plo;
  return a < phi ? a : phi;
}
// fp32(fp64(lo) + pos w)
__host__ __device__ inline float qmap_node(float lo, double pos, double w) {
#pragma clang fp contract(off)
  const double m = pos * w;
  const double e = (double)lo + m;
  return (float)e;
}
__host__ __device__ inline float qmap_sub(float a, float b) {
#pragma clang fp contract(off)
  const float d = a - b;
  return d;
}
// One value through the transfer function node(0 .. nbins + 2) of its pixel: t and the row as hist_bin makes them.
template <typename F>
__host__ __device__ inline float qmap_value(float y, float lo, float inv_w, int nbins, F&& node) {
#pragma clang fp contract(off)
  const float d = y - lo;
  const float t = d * inv_w;
  const bool inner = t >= 0.f && t < (float)nbins;                          // false for NaN
  const int k = (int)(inner ? t : 0.f);
  const float n0 = node(t < 0.f ? nbins + 1 : inner ? k : nbins + 2);       // d_lo, the node below, or d_hi
  const float n1 = node(k + 1);
  const float f = t - (float)k;
  const float dm = n1 - n0;
  const float m = f * dm;
  const float in = n0 + m;
  const float out = y + n0;
  const float v = inner ? in : out;
  return t != t ? __builtin_bit_cast(float, 0x7fc00000u) : v;
}

bool fit_ok(const void* counts, int nout, int nbins, int P, const float* lo, const double* width, const void* nodes) {
  if (!counts || !lo || !width || !nodes || nout < 1 || nout > MAXO || nbins < 1 || nbins > DG_GRIDHIST_MAX_BINS || P < 1) return false;
  for (int j = 0; j < nout; ++j)
    if (!hist_finite(lo[j]) || !(width[j] > 0.0 && width[j] <= DBL_MAX)) return false;
  return true;
}

bool spec_ok(const dg_hist_spec* s, int C) {                         // the checks of dg_gridhist
  if (!s || s->nbins < 1 || s->nbins > DG_GRIDHIST_MAX_BINS || !hist_xform_ok(s, C)) return false;
  for (int j = 0; j < hist_nout(s, C); ++j)
    if (!hist_finite(s->lo[j]) || !(s->inv_w[j] > 0.f && s->inv_w[j] <= FLT_MAX)) return false;
  return true;
}

// ---- fit ------------------------------------------------------------------------------------------------------------------------
struct QfSpec {
  float lo[MAXO];
  double w[MAXO];
};

template <int NPX> struct QRow { int v[NPX]; };
template <int NPX>
__device__ __forceinline__ QRow<NPX> qf_load(const int* q) {
  QRow<NPX> r;
  if constexpr (NPX == 4) {
    const int4 t = *reinterpret_cast<const int4*>(q);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *q;
  }
  return r;
}
template <int NPX>
__device__ __forceinline__ void qf_store(float* q, const float (&v)[NPX]) {
  if constexpr (NPX == 4) st4(q, v);
  else *q = v[0];
}

// The merge walk of one pixel.  b: the pixel's column of the real side (stride P).  s walks 1 .. nbins with B_{s-1} and b[s] at
// hand; h walks -1 .. nbins with B_h and b[h + 1] at hand; neither ever reads beyond row nbins.
struct QWalk {
  long long ng, nr, G, Bsm1, Bh, B0, Bnb;
  int s, bs, h, bn;
  __device__ __forceinline__ void init(const int* b, long long P, long long ng_, long long nr_, long long Bnb_) {
    ng = ng_; nr = nr_; Bnb = Bnb_; G = 0;
    B0 = b[0];
    Bsm1 = B0; s = 1; bs = b[P];
    Bh = 0; h = -1; bn = (int)B0;
  }
  __device__ __forceinline__ double pos(int k, int ak, const int* b, long long P, int nbins) {
    G += ak;
    if (ng == 0 || nr == 0) return (double)k;
    const long long X = G * nr;
    while (h < nbins && (Bh + bn) * ng <= X) {
      ++h;
      Bh += bn;
      bn = h < nbins ? b[(long long)(h + 1) * P] : 0;
    }
    if (X > Bnb * ng) return (double)nbins;
    if (X <= B0 * ng) return qmap_clamp(k, 0.0, (double)(h < 0 ? 0 : h));
    while (s < nbins && (Bsm1 + bs) * ng < X) {
      Bsm1 += bs;
      ++s;
      bs = b[(long long)s * P];
    }
    const double plo = qmap_plo(s, X - Bsm1 * ng, (long long)bs * ng);
    const double phi = plo > (double)h ? plo : (double)h;
    return qmap_clamp(k, plo, phi);
  }
};

template <int NPX>
__global__ __launch_bounds__(QF_THREADS) void qmap_fit_kernel(const int* counts, int nbins, long long P, QfSpec sp, float* nodes) {
  const long long i = (long long)blockIdx.x * QF_THREADS + threadIdx.x;
  if (i >= P / NPX) return;
  const long long p0 = i * NPX, j = blockIdx.y;
  const int nb3 = nbins + 3;
  const int* cb = counts + j * 2 * nb3 * P + p0;                     // side 0: real, the target
  const int* ca = cb + nb3 * P;                                      // side 1: generated, the source
  long long ng[NPX], nr[NPX], Bnb[NPX];
#pragma unroll
  for (int k = 0; k < NPX; ++k) ng[k] = nr[k] = Bnb[k] = 0;
  for (int r = 0; r < nbins + 2; ++r) {
    const QRow<NPX> a = qf_load<NPX>(ca + r * P), b = qf_load<NPX>(cb + r * P);
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      ng[k] += a.v[k];
      nr[k] += b.v[k];
      if (r == nbins) Bnb[k] = nr[k];
    }
  }
  QWalk w[NPX];
#pragma unroll
  for (int k = 0; k < NPX; ++k) w[k].init(cb + k, P, ng[k], nr[k], Bnb[k]);
  const float lo = sp.lo[j];
  const double wd = sp.w[j];
  float* out = nodes + j * nb3 * P + p0;
  float first[NPX], last[NPX];
  for (int e = 0; e <= nbins; ++e) {
    const QRow<NPX> a = qf_load<NPX>(ca + e * P);
    float v[NPX];
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      v[k] = qmap_node(lo, w[k].pos(e, a.v[k], cb + k, P, nbins), wd);
      if (e == 0) first[k] = v[k];
      last[k] = v[k];
    }
    qf_store<NPX>(out + e * P, v);
  }
  const float hi = qmap_node(lo, (double)nbins, wd);
  float dlo[NPX], dhi[NPX];
#pragma unroll
  for (int k = 0; k < NPX; ++k) {
    dlo[k] = qmap_sub(first[k], lo);
    dhi[k] = qmap_sub(last[k], hi);
  }
  qf_store<NPX>(out + (long long)(nbins + 1) * P, dlo);
  qf_store<NPX>(out + (long long)(nbins + 2) * P, dhi);
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------
struct QaArgs {
  HistSeries x;
  int P, T, nout, nbins;
  HistXform xf;
  float lo[MAXO], inv_w[MAXO];
  int slices;
  const float* nodes;
  float* out;
};

// the fields t0 + wave, t0 + wave + QA_WAVES, .. < t1 of this lane's pixel p through the staged transfer function of channel un.j
template <typename T, int MODE, bool SPD>
__device__ __forceinline__ void qa_stream(const QaArgs& g, const HistUnit (&un)[1], float lo, float inv_w, const float* tf, long long p,
                                          long long t0, long long t1) {
  const long long P = g.P;
  float* out = g.out + (long long)un[0].j * P + p;
  const long long ld_o = (long long)g.nout * P;
  auto node = [&](int r) { return tf[r * QA_PX]; };
  auto one = [&](const HistRaw<MODE, 1>& r, long long t) {
    out[t * ld_o] = qmap_value(hist_unit_value<T, MODE, 1, SPD>(r, un[0], 0), lo, inv_w, g.nbins, node);
  };
  long long t = t0;
  for (; t + (QA_UNROLL - 1) * QA_WAVES < t1; t += QA_UNROLL * QA_WAVES) {
    HistRaw<MODE, 1> r[QA_UNROLL];
#pragma unroll
    for (int u = 0; u < QA_UNROLL; ++u) hist_unit_load<T, MODE, 1, SPD>(g.x, t + u * QA_WAVES, p, un, r[u]);
#pragma unroll
    for (int u = 0; u < QA_UNROLL; ++u) one(r[u], t + u * QA_WAVES);
  }
  for (; t < t1; t += QA_WAVES) {
    HistRaw<MODE, 1> r;
    hist_unit_load<T, MODE, 1, SPD>(g.x, t, p, un, r);
    one(r, t);
  }
}

template <typename T, int MODE>
__global__ __launch_bounds__(QA_THREADS) void qmap_apply_kernel(QaArgs g) {
  extern __shared__ __attribute__((aligned(16))) float qa_tf[];      // [nbins + 3][QA_PX]
  const int lane = threadIdx.x % QA_PX, wave = threadIdx.x / QA_PX;
  const long long p = (long long)blockIdx.x * QA_PX + lane, P = g.P;
  const bool live = p < P;                                           // no early return: every lane reaches the barriers
  const long long slice = blockIdx.y;
  const long long t0 = slice * g.T / g.slices, t1 = (slice + 1) * g.T / g.slices;
  const int nb3 = g.nbins + 3;
  for (int j = 0; j < g.nout; ++j) {
    if (j > 0) __syncthreads();                                      // the last channel's nodes are still being read
    const float* src = g.nodes + (long long)j * nb3 * P + p;
    for (int r = wave; r < nb3; r += QA_WAVES) qa_tf[r * QA_PX + lane] = live ? src[(long long)r * P] : 0.f;
    __syncthreads();
    if (!live) continue;
    HistUnit un[1];
    HistUnit& w = un[0];
    w.on = true;
    w.j = j;
    w.spd = g.xf.speed && j == g.xf.C;
    w.c1 = w.spd ? g.xf.su : j;
    w.c2 = w.spd ? g.xf.sv : j;
    w.sc1 = g.xf.scale[w.c1]; w.of1 = g.xf.offset[w.c1];
    w.sc2 = g.xf.scale[w.c2]; w.of2 = g.xf.offset[w.c2];
    if (w.spd)
      qa_stream<T, MODE, true>(g, un, g.lo[j], g.inv_w[j], qa_tf + lane, p, t0 + wave, t1);
    else
      qa_stream<T, MODE, false>(g, un, g.lo[j], g.inv_w[j], qa_tf + lane, p, t0 + wave, t1);
  }
}

// slices of the fields: one when the pixels alone fill the chip, else enough to, of QA_SLICE_MIN_T fields at least
int qa_slices(int T, long long P) {
  const long long nb = (P + QA_PX - 1) / QA_PX;
  if (nb >= QA_BLOCKS_FULL) return 1;
  const long long want = (QA_BLOCKS_FULL + nb - 1) / nb, cap = T / QA_SLICE_MIN_T;
  const long long s = want < cap ? want : cap;
  return (int)(s < 1 ? 1 : s);
}

template <typename T, int MODE>
int qa_launch(const QaArgs& g, hipStream_t st) {
  const int lds = (g.nbins + 3) * QA_PX * (int)sizeof(float);        // 66304 bytes at nbins = 256
  // the opt-in is made once per instance and device, so it asks for the largest table any later call may need, not this call's
  constexpr int LDS_MAX = (DG_GRIDHIST_MAX_BINS + 3) * QA_PX * (int)sizeof(float);
  if (lds > 65536) DG_SET_MAX_LDS_ONCE((&qmap_apply_kernel<T, MODE>), LDS_MAX);
  const dim3 grid((unsigned)(((long long)g.P + QA_PX - 1) / QA_PX), (unsigned)g.slices);
  hipLaunchKernelGGL((qmap_apply_kernel<T, MODE>), grid, dim3(QA_THREADS), lds, st, g);
  return dg_check_launch();
}

}  // namespace

extern "C" int dg_qmap_fit(const int32_t* counts, int nout, int nbins, int P, const float* lo, const double* width, float* nodes,
                           void* stream) {
  if (!fit_ok(counts, nout, nbins, P, lo, width, nodes)) return DG_ERR_BAD_SHAPE;
  QfSpec sp;
  for (int j = 0; j < MAXO; ++j) {
    sp.lo[j] = j < nout ? lo[j] : 0.f;
    sp.w[j] = j < nout ? width[j] : 1.0;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // four pixels per lane when every row of the table and of the nodes is aligned for 16-byte accesses
  const bool quad = P % 4 == 0 && reinterpret_cast<uintptr_t>(counts) % 16 == 0 && reinterpret_cast<uintptr_t>(nodes) % 16 == 0;
  const long long items = quad ? P / 4 : P;
  const dim3 grid((unsigned)((items + QF_THREADS - 1) / QF_THREADS), (unsigned)nout);
  if (quad) hipLaunchKernelGGL(qmap_fit_kernel<4>, grid, dim3(QF_THREADS), 0, st, counts, nbins, (long long)P, sp, nodes);
  else hipLaunchKernelGGL(qmap_fit_kernel<1>, grid, dim3(QF_THREADS), 0, st, counts, nbins, (long long)P, sp, nodes);
  return dg_check_launch();
}

extern "C" int dg_qmap_apply(const dg_eof_fields* x, const dg_hist_spec* s, const float* nodes, float* out, void* stream) {
  if (!hist_fields_ok(x) || !spec_ok(s, x->C) || !nodes || !out) return DG_ERR_BAD_SHAPE;
  if (x->dtype != DG_F32 && x->dtype != DG_BF16) return DG_ERR_BAD_DTYPE;
  QaArgs g;
  g.x = hist_series(x);
  g.xf = hist_xform(s, x->C);
  g.P = x->P; g.T = x->T; g.nout = hist_nout(s, x->C); g.nbins = s->nbins;
  for (int j = 0; j < MAXO; ++j) {
    g.lo[j] = j < g.nout ? s->lo[j] : 0.f;
    g.inv_w[j] = j < g.nout ? s->inv_w[j] : 1.f;
  }
  g.slices = qa_slices(x->T, x->P);
  g.nodes = nodes;
  g.out = out;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // a lane owns one pixel: NCHW planes are read element by element, a wave's 64 elements contiguous
  return hist_dispatch<false>(x->dtype, hist_mode(x), [&](auto t, auto m) { return qa_launch<decltype(t), decltype(m)::value>(g, st); });
}

extern "C" int dg_qmap_fit_host(const int32_t* counts, int nout, int nbins, int P, const float* lo, const double* width, float* nodes) {
  if (!fit_ok(counts, nout, nbins, P, lo, width, nodes)) return DG_ERR_BAD_SHAPE;
  const int64_t nb3 = nbins + 3, Pl = P;
  std::vector<long long> Bs((size_t)nbins + 1);
  for (int64_t j = 0; j < nout; ++j)
    for (int64_t p = 0; p < Pl; ++p) {
      const int32_t* b = counts + j * 2 * nb3 * Pl + p;              // real
      const int32_t* a = b + nb3 * Pl;                               // generated
      float* o = nodes + j * nb3 * Pl + p;
      long long ng = 0, nr = 0;
      for (int r = 0; r < nbins + 2; ++r) { ng += a[r * Pl]; nr += b[r * Pl]; }
      // B'_s in an array, searched from the start for every k: the definition itself, no pointer carried from k to k + 1
      long long c = 0;
      for (int s = 0; s <= nbins; ++s) { c += b[s * Pl]; Bs[s] = c * ng; }
      auto Bp = [&](int s) { return Bs[s]; };
      long long G = 0;
      for (int k = 0; k <= nbins; ++k) {
        G += a[k * Pl];
        double pos = (double)k;
        if (ng != 0 && nr != 0) {
          const long long X = G * nr;
          int top = -1;                                              // max{s : B'_s <= X}
          for (int s = 0; s <= nbins; ++s)
            if (Bp(s) <= X) top = s;
          if (X > Bp(nbins)) {
            pos = (double)nbins;
          } else if (X <= Bp(0)) {
            pos = qmap_clamp(k, 0.0, (double)(top < 0 ? 0 : top));
          } else {
            int s = 1;
            while (Bp(s) < X) ++s;
            const double plo = qmap_plo(s, X - Bp(s - 1), (long long)b[s * Pl] * ng);
            pos = qmap_clamp(k, plo, plo > (double)top ? plo : (double)top);
          }
        }
        o[k * Pl] = qmap_node(lo[j], pos, width[j]);
      }
      o[(nbins + 1) * Pl] = qmap_sub(o[0], lo[j]);
      o[(nbins + 2) * Pl] = qmap_sub(o[nbins * Pl], qmap_node(lo[j], (double)nbins, width[j]));
    }
  return DG_OK;
}

extern "C" int dg_qmap_apply_host(const dg_hist_spec* s, const float* x, int C, int T, int P, const float* nodes, float* out) {
  if (!spec_ok(s, C) || T < 1 || P < 1 || !x || !nodes || !out) return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C);
  const int64_t nb3 = s->nbins + 3, Pl = P;
  for (int64_t t = 0; t < T; ++t)
    for (int j = 0; j < nout; ++j)
      for (int64_t p = 0; p < Pl; ++p) {
        const float* tf = nodes + j * nb3 * Pl + p;
        const float y = hist_host_value(s, x + t * C * Pl, C, (size_t)P, (size_t)p, j);
        out[(t * nout + j) * Pl + p] = qmap_value(y, s->lo[j], s->inv_w[j], s->nbins, [&](int r) { return tf[r * Pl]; });
      }
  return DG_OK;
}
