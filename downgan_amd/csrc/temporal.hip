// Temporal diagnostics (include/downgan_hip.h "Temporal diagnostics") of one or two series of fields in time order, read through
// the EOF descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16): spell durations per threshold, ramp histograms per lag and the
// sums of the lag autocorrelation per gridpoint, with the open run and the last R values of every pixel carried from call to call.
//   temporal_kernel<T, MODE, SPD>
//       one launch per series and per class of output channel (SPD: the speed channel, which loads two input channels;
//       blockIdx.y = the output channel otherwise).  A thread owns four consecutive pixels of an NCHW plane (MODE = HIST_NCHW4: one
//       16 B / 8 B load per plane and field; only on grids that fill the chip that way) or one pixel (HIST_PIX16 = one 16-byte
//       load per field, HIST_ANY = one element per load); a wave's pixels are contiguous, so the state rows [..][P] are read and
//       written coalesced.  The thread walks ALL fields of the call in t order -- the time axis is never cut, which is what makes
//       the result independent of the chunking -- TP_U fields in flight before the first is consumed, with the open runs, the
//       per-pixel counts and the fp64 sums in registers.  y[t - tau] is not kept in a register window (a window indexed by a
//       run-time lag is a dynamically indexed register array): field t - tau of the same call is loaded again and transformed
//       again -- it was read tau steps ago by the same wave, so the caches serve it -- and for t - tau < t0 the value comes from
//       the tail ring, which the thread itself rewrites during the last R steps (a slot is always read before the step that
//       overwrites it: see the note at the store).  The pooled tables are uint32 LDS tables (ds_add_u32), flushed once with
//       64-bit integer atomics.  No float atomics, no data-dependent trip count.
// A launch takes at most TP_TMAX fields so that no uint32 cell can wrap; longer calls are cut into launches on the host, which
// the chunking contract makes invisible.
#include <float.h>
#include <math.h>

#include <vector>

#include "dg_internal.h"
#include "hist_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_TMAX = 1 << 20;                      // fields per launch: 256 threads * 4 pixels * 2^20 adds < 2^32 per LDS cell
constexpr long long TP_QUAD_MIN_ITEMS = 65536;        // four pixels per thread only where P / 4 still gives every CU a workgroup
constexpr int MAXO = DG_HIST_MAX_OUT, MAXK = DG_TEMPORAL_MAX_THR, MAXL = DG_TEMPORAL_MAX_LAGS;
constexpr int MAXB3 = DG_TEMPORAL_MAX_BINS + 3, MAXD = DG_TEMPORAL_MAX_DUR;

struct TpArgs {
  HistSeries x;
  HistXform xf;
  int P, T;
  int nthr, ndur, nlag, nbins, R;
  int t0, slot0;                                      // the absolute time of the launch's first field; t0 mod R
  int below[MAXK], lag[MAXL];
  float thr[MAXO][MAXK], lo[MAXO][MAXL], inv_w[MAXO][MAXL];
  // the arrays of this launch's series
  int* open;
  float* tail;
  unsigned long long* spells;
  int* spellmap;
  unsigned long long* ramps;
  double* acsum;
  int* accnt;
};

// the loads of one field for this thread's pixels: the raw input, or (from the tail ring) y itself in x1
template <int MODE, bool SPD> struct TpRaw {
  static constexpr int NPX = MODE == HIST_NCHW4 ? 4 : 1;
  float x1[NPX], x2[SPD ? NPX : 1];
};
template <bool SPD> struct TpRaw<HIST_PIX16, SPD> { uint4 r; };

// field tl (index within the launch) of this thread's pixels (i: pixel quad in HIST_NCHW4, else pixel)
template <typename T, int MODE, bool SPD>
__device__ __forceinline__ void tp_load(const TpArgs& g, long long tl, long long i, int c1, int c2, TpRaw<MODE, SPD>& r) {
  const T* base = reinterpret_cast<const T*>(g.x.base) + tl * g.x.ld_t;
  if constexpr (MODE == HIST_NCHW4) {
    ld4(base + c1 * g.x.ld_c + 4 * i, r.x1);
    if constexpr (SPD) ld4(base + c2 * g.x.ld_c + 4 * i, r.x2);
  } else if constexpr (MODE == HIST_PIX16) {
    r.r = *reinterpret_cast<const uint4*>(base + i * g.x.ld_p);
  } else {
    r.x1[0] = ld_elem(base + c1 * g.x.ld_c + i * g.x.ld_p);
    if constexpr (SPD) r.x2[0] = ld_elem(base + c2 * g.x.ld_c + i * g.x.ld_p);
  }
}

// y of ring row `row` (this output channel's [R][P] + slot * P) at this thread's pixels
template <int MODE, bool SPD>
__device__ __forceinline__ void tp_load_ring(const float* row, long long p0, TpRaw<MODE, SPD>& r) {
  if constexpr (MODE == HIST_PIX16) {
    r.r.x = __float_as_uint(row[p0]);
  } else {
#pragma unroll
    for (int q = 0; q < TpRaw<MODE, SPD>::NPX; ++q) r.x1[q] = row[p0 + q];
  }
}

struct TpXf { int c1, c2; float sc1, of1, sc2, of2; };

// the output value of pixel q of a load (ring: the load holds y already)
template <typename T, int MODE, bool SPD>
__device__ __forceinline__ float tp_value(const TpRaw<MODE, SPD>& r, int q, bool ring, const TpXf& x) {
  float x1, x2;
  if constexpr (MODE == HIST_PIX16) {
    if (ring) return __uint_as_float(r.r.x);
    x1 = hist_pick16_sel<T>(r.r, x.c1);
    x2 = SPD ? hist_pick16_sel<T>(r.r, x.c2) : x1;
  } else {
    if (ring) return r.x1[q];
    x1 = r.x1[q];
    x2 = SPD ? r.x2[SPD ? q : 0] : x1;
  }
  const float y = hist_affine(x1, x.sc1, x.of1);
  return SPD ? hist_speed(y, hist_affine(x2, x.sc2, x.of2)) : y;
}

template <typename T, int MODE, bool SPD>
__global__ __launch_bounds__(TP_THREADS) void temporal_kernel(TpArgs g) {
  constexpr int NPX = MODE == HIST_NCHW4 ? 4 : 1;
  constexpr int TP_U = NPX == 4 ? 2 : 4;              // fields in flight (each with its nlag partners)
  __shared__ unsigned int lds_ramps[MAXL * MAXB3];
  __shared__ unsigned int lds_spells[MAXK * MAXD];
  const int tid = threadIdx.x, nb3 = g.nbins + 3;
  for (int i = tid; i < g.nlag * nb3; i += TP_THREADS) lds_ramps[i] = 0u;
  for (int i = tid; i < g.nthr * g.ndur; i += TP_THREADS) lds_spells[i] = 0u;
  __syncthreads();

  const int j = SPD ? g.xf.C : (int)blockIdx.y;          // the output channel of this workgroup
  const long long P = g.P, i = (long long)blockIdx.x * TP_THREADS + tid, p0 = i * NPX;
  if (i < P / NPX) {
    TpXf xf;
    xf.c1 = SPD ? g.xf.su : j;
    xf.c2 = SPD ? g.xf.sv : j;
    xf.sc1 = g.xf.scale[xf.c1]; xf.of1 = g.xf.offset[xf.c1];
    xf.sc2 = g.xf.scale[xf.c2]; xf.of2 = g.xf.offset[xf.c2];
    float thr[MAXK], lo[MAXL], inv_w[MAXL];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) thr[k] = g.thr[j][k];
#pragma unroll
    for (int l = 0; l < MAXL; ++l) { lo[l] = g.lo[j][l]; inv_w[l] = g.inv_w[j][l]; }

    // the rows of this output channel
    int* open = g.open + (long long)j * g.nthr * P + p0;                      // [nthr][P]
    int* smap = g.spellmap + (long long)j * g.nthr * 3 * P + p0;              // [nthr][3][P]
    float* tail = g.tail + (long long)j * g.R * P;                            // [R][P] (indexed with p0 + q)
    double* acsum = g.acsum + (long long)j * (2 + 2 * g.nlag) * P + p0;       // [2 + 2 nlag][P]
    int* accnt = g.accnt + (long long)j * (1 + g.nlag) * P + p0;              // [1 + nlag][P]

    int run[MAXK][NPX], ncomp[MAXK][NPX], total[MAXK][NPX], longest[MAXK][NPX];
    int n[NPX], m[MAXL][NPX];
    double s1[NPX], s2[NPX], cs[MAXL][NPX], es[MAXL][NPX];
#pragma unroll
    for (int q = 0; q < NPX; ++q) {
#pragma unroll
      for (int k = 0; k < MAXK; ++k) {
        const bool on = k < g.nthr;
        run[k][q] = on ? open[k * P + q] : 0;
        longest[k][q] = on ? smap[(k * 3 + 2) * P + q] : 0;
        ncomp[k][q] = 0;
        total[k][q] = 0;
      }
      n[q] = accnt[q];
      s1[q] = acsum[q];
      s2[q] = acsum[P + q];
#pragma unroll
      for (int l = 0; l < MAXL; ++l) {
        const bool on = l < g.nlag;
        m[l][q] = on ? accnt[(1 + l) * P + q] : 0;
        cs[l][q] = on ? acsum[(2 + 2 * l) * P + q] : 0.0;
        es[l][q] = on ? acsum[(3 + 2 * l) * P + q] : 0.0;
      }
    }

    for (int tb = 0; tb < g.T; tb += TP_U) {
      TpRaw<MODE, SPD> cur[TP_U], par[TP_U][MAXL];
#pragma unroll
      for (int u = 0; u < TP_U; ++u) {
        const int t = tb + u;
        if (t < g.T) {
          tp_load<T, MODE, SPD>(g, t, i, xf.c1, xf.c2, cur[u]);
#pragma unroll
          for (int l = 0; l < MAXL; ++l) {
            if (l < g.nlag && g.t0 + t - g.lag[l] >= 0) {                     // wave-uniform
              if (t - g.lag[l] >= 0)
                tp_load<T, MODE, SPD>(g, t - g.lag[l], i, xf.c1, xf.c2, par[u][l]);
              else
                tp_load_ring<MODE, SPD>(tail + (long long)((g.slot0 + t - g.lag[l] + g.R) % g.R) * P, p0, par[u][l]);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < TP_U; ++u) {
        const int t = tb + u;
        if (t < g.T) {
          const bool keep = g.nlag > 0 && t >= g.T - g.R;                     // one of the last R fields: into the ring
          float* slot = tail + (long long)(g.nlag > 0 ? (g.slot0 + t) % g.R : 0) * P + p0;
#pragma unroll
          for (int q = 0; q < NPX; ++q) {
            const float y = tp_value<T, MODE, SPD>(cur[u], q, false, xf);
            const bool fin = hist_finite(y);
            const double yd = (double)y;
#pragma unroll
            for (int k = 0; k < MAXK; ++k) {
              if (k < g.nthr) {
                const bool cond = g.below[k] ? y < thr[k] : y > thr[k];
                const int r = run[k][q];
                const bool end = !cond && r > 0;
                if (end) atomicAdd(&lds_spells[k * g.ndur + min(r, g.ndur) - 1], 1u);
                ncomp[k][q] += end ? 1 : 0;
                total[k][q] += end ? r : 0;
                const int r1 = cond ? r + 1 : 0;
                longest[k][q] = max(longest[k][q], r1);
                run[k][q] = r1;
              }
            }
            n[q] += fin ? 1 : 0;
            s1[q] = fin ? s1[q] + yd : s1[q];
            s2[q] = fin ? s2[q] + yd * yd : s2[q];
#pragma unroll
            for (int l = 0; l < MAXL; ++l) {
              if (l < g.nlag && g.t0 + t - g.lag[l] >= 0) {
                const float yl = tp_value<T, MODE, SPD>(par[u][l], q, t - g.lag[l] < 0, xf);
                const float d = hist_diff(y, yl);
                atomicAdd(&lds_ramps[l * nb3 + hist_bin(d, lo[l], inv_w[l], g.nbins)], 1u);
                const bool both = fin && hist_finite(yl);
                const double yld = (double)yl;
                m[l][q] += both ? 1 : 0;
                cs[l][q] = both ? cs[l][q] + yd * yld : cs[l][q];
                es[l][q] = both ? es[l][q] + (yd + yld) : es[l][q];
              }
            }
            // Slot (t0 + t) mod R held time t0 + t - R, which only step t itself (lag R) still reads, and that load was issued
            // above: a later step t' > t reads times t' - tau > t - R.  Loads of later steps of this block that were issued
            // before this store read other slots for the same reason.
            if (keep) slot[q] = y;
          }
        }
      }
    }

#pragma unroll
    for (int q = 0; q < NPX; ++q) {
#pragma unroll
      for (int k = 0; k < MAXK; ++k) {
        if (k < g.nthr) {
          open[k * P + q] = run[k][q];
          smap[(k * 3) * P + q] += ncomp[k][q];
          smap[(k * 3 + 1) * P + q] += total[k][q];
          smap[(k * 3 + 2) * P + q] = longest[k][q];
        }
      }
      accnt[q] = n[q];
      acsum[q] = s1[q];
      acsum[P + q] = s2[q];
#pragma unroll
      for (int l = 0; l < MAXL; ++l) {
        if (l < g.nlag) {
          accnt[(1 + l) * P + q] = m[l][q];
          acsum[(2 + 2 * l) * P + q] = cs[l][q];
          acsum[(3 + 2 * l) * P + q] = es[l][q];
        }
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < g.nlag * nb3; c += TP_THREADS) {
    const unsigned v = lds_ramps[c];
    if (v) atomicAdd(g.ramps + (long long)j * g.nlag * nb3 + c, (unsigned long long)v);
  }
  for (int c = tid; c < g.nthr * g.ndur; c += TP_THREADS) {
    const unsigned v = lds_spells[c];
    if (v) atomicAdd(g.spells + (long long)j * g.nthr * g.ndur + c, (unsigned long long)v);
  }
}

bool spec_ok(const dg_temporal_spec* s, int C) {
  if (!s || !hist_xform_ok(s, C)) return false;
  if (s->nthr < 0 || s->nthr > MAXK || s->nlag < 0 || s->nlag > MAXL || (s->nthr == 0 && s->nlag == 0)) return false;
  if (s->ndur < 1 || s->ndur > MAXD || s->nbins < 1 || s->nbins > DG_TEMPORAL_MAX_BINS) return false;
  for (int k = 0; k < s->nthr; ++k)
    if (s->below[k] != 0 && s->below[k] != 1) return false;
  for (int l = 0; l < s->nlag; ++l)
    if (s->lag[l] < 1 || s->lag[l] > DG_TEMPORAL_MAX_LAG || (l > 0 && s->lag[l] <= s->lag[l - 1])) return false;
  const int nout = hist_nout(s, C);
  for (int j = 0; j < nout; ++j)
    for (int l = 0; l < s->nlag; ++l)
      if (!hist_finite(s->lo[j][l]) || !(s->inv_w[j][l] > 0.f && s->inv_w[j][l] <= FLT_MAX)) return false;
  return hist_thr_ok(s->thr, nout, s->nthr);
}

bool time_ok(int64_t t0, int T) { return t0 >= 0 && t0 + (int64_t)T < ((int64_t)1 << 31); }

bool arrays_ok(const dg_temporal_spec* s, const void* open, const void* tail, const void* spells, const void* spellmap,
               const void* ramps, const void* acsum, const void* accnt) {
  if (!acsum || !accnt) return false;
  if (s->nthr > 0 && (!open || !spells || !spellmap)) return false;
  if (s->nlag > 0 && (!tail || !ramps)) return false;
  return true;
}

bool call_ok(const dg_eof_fields* a, const dg_eof_fields* b, const dg_temporal_spec* s) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C)) return false;
  return !b || (hist_fields_ok(b) && b->T == a->T && b->C == a->C && b->P == a->P);
}

bool dtype_ok(const dg_eof_fields* x) { return x->dtype == DG_F32 || x->dtype == DG_BF16; }

template <typename T, int MODE>
void launch_mode(const TpArgs& g, bool speed, hipStream_t st) {
  constexpr int NPX = MODE == HIST_NCHW4 ? 4 : 1;
  const long long items = g.P / NPX;
  const unsigned nbx = (unsigned)((items + TP_THREADS - 1) / TP_THREADS);
  hipLaunchKernelGGL((temporal_kernel<T, MODE, false>), dim3(nbx, (unsigned)g.xf.C), dim3(TP_THREADS), 0, st, g);
  if (speed) hipLaunchKernelGGL((temporal_kernel<T, MODE, true>), dim3(nbx, 1), dim3(TP_THREADS), 0, st, g);
}

}  // namespace

extern "C" size_t dg_temporal_ws_bytes(const dg_eof_fields* a, const dg_eof_fields* b, const dg_temporal_spec* s) {
  return call_ok(a, b, s) ? 256 : 0;                                  // no partial state: every sum has one owner
}

extern "C" int dg_temporal(const dg_eof_fields* a, const dg_eof_fields* b, const dg_temporal_spec* s, int64_t t0, void* ws,
                           int32_t* open, float* tail, int64_t* spells, int32_t* spellmap, int64_t* ramps, double* acsum,
                           int32_t* accnt, void* stream) {
  if (!call_ok(a, b, s) || !time_ok(t0, a->T) || !arrays_ok(s, open, tail, spells, spellmap, ramps, acsum, accnt))
    return DG_ERR_BAD_SHAPE;
  if (!dtype_ok(a) || (b && !dtype_ok(b))) return DG_ERR_BAD_DTYPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool speed = s->speed_u >= 0;
  const long long P = a->P, nout = hist_nout(s, a->C), nb3 = s->nbins + 3;
  const int R = s->nlag > 0 ? s->lag[s->nlag - 1] : 0;

  TpArgs g;
  g.xf = hist_xform(s, a->C);
  g.P = a->P;
  g.nthr = s->nthr; g.ndur = s->ndur; g.nlag = s->nlag; g.nbins = s->nbins; g.R = R;
  for (int k = 0; k < MAXK; ++k) g.below[k] = k < s->nthr ? s->below[k] : 0;
  for (int l = 0; l < MAXL; ++l) g.lag[l] = l < s->nlag ? s->lag[l] : 0;
  for (int j = 0; j < MAXO; ++j) {
    for (int k = 0; k < MAXK; ++k) g.thr[j][k] = j < nout && k < s->nthr ? s->thr[j][k] : 0.f;
    for (int l = 0; l < MAXL; ++l) {
      const bool on = j < nout && l < s->nlag;
      g.lo[j][l] = on ? s->lo[j][l] : 0.f;
      g.inv_w[j][l] = on ? s->inv_w[j][l] : 1.f;
    }
  }
  for (int ser = 0; ser < (b ? 2 : 1); ++ser) {
    const dg_eof_fields* x = ser ? b : a;
    g.x = hist_series(x);
    // the arrays of this series (a NULL array is never touched: its nthr / nlag is 0)
    g.open = open ? open + ser * nout * s->nthr * P : nullptr;
    g.tail = tail ? tail + ser * nout * R * P : nullptr;
    g.spells = spells ? reinterpret_cast<unsigned long long*>(spells) + ser * nout * s->nthr * s->ndur : nullptr;
    g.spellmap = spellmap ? spellmap + ser * nout * s->nthr * 3 * P : nullptr;
    g.ramps = ramps ? reinterpret_cast<unsigned long long*>(ramps) + ser * nout * s->nlag * nb3 : nullptr;
    g.acsum = acsum + ser * nout * (2 + 2 * s->nlag) * P;
    g.accnt = accnt + ser * nout * (1 + s->nlag) * P;
    // four pixels per thread where the planes allow it and the grid is large enough to fill the chip that way
    int mode = hist_mode(x);
    if (mode == HIST_NCHW4 && P / 4 < TP_QUAD_MIN_ITEMS) mode = HIST_ANY;
    const size_t es = x->dtype == DG_F32 ? 4 : 2;
    for (long long tt = 0; tt < x->T; tt += TP_TMAX) {
      g.x.base = static_cast<const char*>(x->base) + (size_t)tt * (size_t)x->ld_t * es;
      g.T = (int)(x->T - tt < TP_TMAX ? x->T - tt : TP_TMAX);
      g.t0 = (int)(t0 + tt);
      g.slot0 = R > 0 ? (int)((t0 + tt) % R) : 0;
      hist_dispatch(x->dtype, mode, [&](auto t, auto m) { launch_mode<decltype(t), decltype(m)::value>(g, speed, st); });
    }
  }
  return dg_check_launch();
}

extern "C" int dg_temporal_host(const dg_temporal_spec* s, const float* x, int C, int T, int P, int64_t t0, int32_t* open,
                                float* tail, int64_t* spells, int32_t* spellmap, int64_t* ramps, double* acsum, int32_t* accnt) {
  if (!spec_ok(s, C) || T < 1 || P < 1 || !x || !time_ok(t0, T) || !arrays_ok(s, open, tail, spells, spellmap, ramps, acsum, accnt))
    return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C), nb3 = s->nbins + 3, nthr = s->nthr, nlag = s->nlag;
  const int R = nlag > 0 ? s->lag[nlag - 1] : 0;
  const size_t Pl = (size_t)P;
  // y of the times t0 - R .. t0 + T - 1 of one output channel and pixel: the ring's part, then this call's
  std::vector<float> y((size_t)R + T);
  for (int j = 0; j < nout; ++j)
    for (size_t p = 0; p < Pl; ++p) {
      for (int64_t ta = t0 - R; ta < t0; ++ta)
        y[(size_t)(ta - (t0 - R))] = ta >= 0 ? tail[((size_t)j * R + (size_t)(ta % R)) * Pl + p] : 0.f;
      for (int t = 0; t < T; ++t) y[(size_t)R + t] = hist_host_value(s, x + (size_t)t * C * Pl, C, Pl, p, j);
      double* sums = acsum + (size_t)j * (2 + 2 * nlag) * Pl + p;
      int32_t* cnt = accnt + (size_t)j * (1 + nlag) * Pl + p;
      for (int t = 0; t < T; ++t) {
        const float yt = y[(size_t)R + t];
        for (int k = 0; k < nthr; ++k) {
          const bool cond = s->below[k] ? yt < s->thr[j][k] : yt > s->thr[j][k];
          int32_t* run = open + ((size_t)j * nthr + k) * Pl + p;
          int32_t* map = spellmap + ((size_t)j * nthr + k) * 3 * Pl + p;
          if (cond) {
            *run += 1;
            if (*run > map[2 * Pl]) map[2 * Pl] = *run;
          } else if (*run > 0) {
            spells[((size_t)j * nthr + k) * s->ndur + (*run < s->ndur ? *run : s->ndur) - 1] += 1;
            map[0] += 1;
            map[Pl] += *run;
            *run = 0;
          }
        }
        const bool fin = hist_finite(yt);
        const double yd = (double)yt;
        if (fin) {
          cnt[0] += 1;
          sums[0] += yd;
          sums[Pl] += yd * yd;
        }
        for (int l = 0; l < nlag; ++l) {
          if (t0 + t - s->lag[l] < 0) continue;
          const float yl = y[(size_t)R + t - s->lag[l]];
          const float d = hist_diff(yt, yl);
          ramps[((size_t)j * nlag + l) * nb3 + hist_bin(d, s->lo[j][l], s->inv_w[j][l], s->nbins)] += 1;
          if (fin && hist_finite(yl)) {
            const double yld = (double)yl;
            cnt[(1 + l) * Pl] += 1;
            sums[(2 + 2 * l) * Pl] += yd * yld;
            sums[(3 + 2 * l) * Pl] += yd + yld;
          }
        }
      }
      for (int t = T > R ? T - R : 0; t < T; ++t)
        tail[((size_t)j * R + (size_t)((t0 + t) % R)) * Pl + p] = y[(size_t)R + t];
    }
  return DG_OK;
}
