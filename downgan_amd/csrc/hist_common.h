// The field reader of the diagnostics: a series of fields in through dg_eof_fields, output values y out.  Twelve translation units
// read fields this way -- the value histograms (histogram.hip), the joint histograms (joint.hip), the per-gridpoint statistics
// (gridstats.hip) and histograms (gridhist.hip), the quantile mapping fitted on them (qmap.hip), the fractions skill score
// (fss.hip), the exceedance objects (objects.hip), the distance maps (distmap.hip), the increment histograms (increments.hip),
// the temporal diagnostics (temporal.hip), the
// intensity-scale verification (iscale.hip) and the field-deformation verification (deform.hip) -- and all must see the same output values y bit for bit, on the device and in their
// host references.  So y is defined here and only here: the arithmetic rules (hist_affine, hist_speed, hist_diff, hist_bin, hist_dir), the load modes and how a pixel is unpacked
// in each, the kernel-argument form of a spec's transform (HistXform) with its padding, the device loaders per access pattern
// (hist_pixel_values, hist_load_item, hist_unit_load / hist_unit_value, hist_pick16_sel), the spec checks and the host value
// (hist_host_value).  DESIGN.md "Field reader" says which loader serves which access pattern.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "dg_internal.h"

// Definition, shared by the kernels and the host reference: each line is one correctly rounded fp32 operation.
__host__ __device__ inline float hist_affine(float x, float scale, float offset) {
#pragma clang fp contract(off)
  const float m = x * scale;
  return m + offset;
}
__host__ __device__ inline float hist_speed(float u, float v) {
#pragma clang fp contract(off)
  const float uu = u * u;
  const float vv = v * v;
  return __builtin_sqrtf(uu + vv);
}
// The increment of the increment histograms (increments.hip): one correctly rounded fp32 subtraction of two already rounded y,
// never contracted with the affine that made them.
__host__ __device__ inline float hist_diff(float y1, float y0) {
#pragma clang fp contract(off)
  const float d = y1 - y0;
  return d;
}
// The bin rule of the definition: each line is one correctly rounded fp32 operation.
__host__ __device__ inline int hist_bin(float y, float lo, float inv_w, int nbins) {
#pragma clang fp contract(off)
  const float d = y - lo;
  const float t = d * inv_w;
  const bool inner = t >= 0.f && t < (float)nbins;                          // false for NaN
  const int b = t < 0.f ? 0 : t >= (float)nbins ? nbins + 1 : 1 + (int)(inner ? t : 0.f);   // selects, not branches; only an
  return t != t ? nbins + 2 : b;                                            // in-range t is converted (anything else is undefined in C++)
}
// The direction rule of the joint histograms (include/downgan_hip.h "Joint histograms", steps 1-8): the index of the sector the
// wind (yu, yv) of speed s comes from; K = nsec / 4, tan_k[k] = fp32(tan(k pi / (4 K))), k = 1 .. K-1.  No atan2: compares of
// one rounded product each.
__host__ __device__ inline int hist_dir(float yu, float yv, float s, float calm, int K, const float* tan_k) {
#pragma clang fp contract(off)
  if (yu != yu || yv != yv) return 4 * K + 2;
  if (!(s > calm)) return 0;
  const float x = -yu, y = -yv;
  const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
  const bool swap = ax > ay;
  const float m = swap ? ay : ax, M = swap ? ax : ay;
  int j = 0;
  for (int k = 1; k < K; ++k) {
    const float e = M * tan_k[k];
    j += m >= e ? 1 : 0;
  }
  const int q = swap ? 2 * K - 1 - j : j;
  const int h = x >= 0.f && y > 0.f ? q : x > 0.f && y <= 0.f ? 4 * K - 1 - q : x <= 0.f && y < 0.f ? 4 * K + q : 8 * K - 1 - q;
  const int sec = (h + 1) >> 1;
  return 1 + (sec >= 4 * K ? sec - 4 * K : sec);
}

// Load modes: HIST_NCHW4 = four consecutive pixels of one NCHW plane per load (16 B fp32, 8 B bf16); HIST_PIX16 = one 16-byte
// load per pixel (the generator's [B, H, W, 16] bf16 output: 8 channels); HIST_ANY = one element per load (any strides).
constexpr int HIST_NCHW4 = 0, HIST_PIX16 = 1, HIST_ANY = 2;
constexpr int HIST_MAXC = DG_EOF_MAX_C, HIST_MAXO = DG_HIST_MAX_OUT;

inline bool hist_fields_ok(const dg_eof_fields* x) {
  return x && x->base && x->T >= 1 && x->C >= 1 && x->C <= DG_EOF_MAX_C && x->P >= 1 && x->ld_t >= 0 && x->ld_c >= 0 && x->ld_p >= 0;
}

inline int hist_mode(const dg_eof_fields* x) {
  const size_t es = x->dtype == DG_F32 ? 4 : 2;
  const uintptr_t b = reinterpret_cast<uintptr_t>(x->base);
  if (x->ld_p == 1 && x->P % 4 == 0 && x->ld_t % 4 == 0 && x->ld_c % 4 == 0 && b % (4 * es) == 0) return HIST_NCHW4;
  if (x->ld_c == 1 && x->ld_p * es >= 16 && (x->ld_p * es) % 16 == 0 && (size_t)x->C * es <= 16 && (x->ld_t * es) % 16 == 0 && b % 16 == 0)
    return HIST_PIX16;
  return HIST_ANY;
}

// One series as a kernel argument.
struct HistSeries {
  const void* base;
  long long ld_t, ld_c, ld_p;
};
inline HistSeries hist_series(const dg_eof_fields* x) { return HistSeries{x->base, x->ld_t, x->ld_c, x->ld_p}; }

// ---- the transform of a spec: checks, kernel-argument form, host value ---------------------------------------------------------
// Every public spec struct names the members speed_u, speed_v, scale, offset: the functions below take any of them.

__host__ __device__ inline bool hist_finite(float v) { return __builtin_fabsf(v) <= FLT_MAX; }   // false for NaN and +-inf

// output channels: the C input channels, and the speed appended as channel C
template <typename S> inline int hist_nout(const S* s, int C) { return C + (s->speed_u >= 0 ? 1 : 0); }

// the channel count, the speed-pair rule (both channels or neither, below C) and finite scale / offset
template <typename S> inline bool hist_xform_ok(const S* s, int C) {
  if (C < 1 || C > HIST_MAXC) return false;
  const bool speed = s->speed_u >= 0 || s->speed_v >= 0;
  if (speed && (s->speed_u < 0 || s->speed_u >= C || s->speed_v < 0 || s->speed_v >= C)) return false;
  for (int c = 0; c < C; ++c)
    if (!hist_finite(s->scale[c]) || !hist_finite(s->offset[c])) return false;
  return true;
}

// the first nthr thresholds of the first nout output channels are finite
template <int K> inline bool hist_thr_ok(const float (&thr)[HIST_MAXO][K], int nout, int nthr) {
  for (int j = 0; j < nout; ++j)
    for (int k = 0; k < nthr; ++k)
      if (!hist_finite(thr[j][k])) return false;
  return true;
}

// The transform as a kernel argument.  Beyond C, scale is 1 and offset 0; without a speed channel su = sv = -1, which no channel
// index equals.  (Four of the kernels used to pass 0 there, and histogram.hip the spec's own speed_u / speed_v, any negative
// values: hist_xform_ok lets both be >= 0 or both < 0, and no c in 0 .. 7 equals a negative one, so -1 selects what they
// selected.  None of the nine reads su / sv unless the speed is on: the selects `c == su` of hist_pixel_values, histogram.hip and
// joint.hip feed a value that is used under `speed` / an axis on channel >= C alone, and the unit kernels, increments.hip and
// temporal.hip take su / sv for the speed channel only, which exists with speed_u >= 0 only.  So one convention serves all.)  The member order is not free: the kernels that take it run at the SGPR limit,
// and with C in front gridhist_kernel gained a 20-byte private segment in two instantiations (DESIGN.md "Field reader").
struct HistXform {
  int speed, su, sv, C;
  float scale[HIST_MAXC], offset[HIST_MAXC];
};
template <typename S> inline HistXform hist_xform(const S* s, int C) {
  HistXform xf;
  xf.C = C;
  xf.speed = s->speed_u >= 0 ? 1 : 0;
  xf.su = xf.speed ? s->speed_u : -1;
  xf.sv = xf.speed ? s->speed_v : -1;
  for (int c = 0; c < HIST_MAXC; ++c) {
    xf.scale[c] = c < C ? s->scale[c] : 1.f;
    xf.offset[c] = c < C ? s->offset[c] : 0.f;
  }
  return xf;
}

// thresholds as a kernel argument: +inf (never exceeded) beyond nout / nthr
template <int K> inline void hist_thr_pad(const float (&thr)[HIST_MAXO][K], int nout, int nthr, float (&out)[HIST_MAXO][K]) {
  for (int j = 0; j < HIST_MAXO; ++j)
    for (int k = 0; k < K; ++k) out[j][k] = j < nout && k < nthr ? thr[j][k] : INFINITY;
}

// Host reference: output channel j of pixel p of one planar fp32 field x[C][P]
template <typename S> inline float hist_host_value(const S* s, const float* x, int C, size_t P, size_t p, int j) {
  if (j < C) return hist_affine(x[j * P + p], s->scale[j], s->offset[j]);
  const int u = s->speed_u, v = s->speed_v;
  return hist_speed(hist_affine(x[u * P + p], s->scale[u], s->offset[u]), hist_affine(x[v * P + p], s->scale[v], s->offset[v]));
}

inline size_t hist_round256(size_t n) { return (n + 255) / 256 * 256; }

// dtype x load mode -> f(T{}, std::integral_constant<int, MODE>{}), T = float / bf16_t (the caller has checked the dtype).
// QUAD = false: for kernels without a four-pixel path, HIST_NCHW4 planes are read element by element (HIST_ANY).
// A call site passes a generic lambda and reads the two tags back as template arguments:
//   hist_dispatch(x->dtype, mode, [&](auto t, auto m) { return launch<decltype(t), decltype(m)::value>(args...); });
// decltype(t) is the element type, decltype(m)::value the HIST_* constant; the values t and m themselves carry nothing.
template <bool QUAD, typename T, typename F> inline auto hist_dispatch_mode(int mode, F&& f) {
  if constexpr (QUAD) {
    if (mode == HIST_NCHW4) return f(T{}, std::integral_constant<int, HIST_NCHW4>{});
  }
  if (mode == HIST_PIX16) return f(T{}, std::integral_constant<int, HIST_PIX16>{});
  return f(T{}, std::integral_constant<int, HIST_ANY>{});
}
template <bool QUAD = true, typename F> inline auto hist_dispatch(int dtype, int mode, F&& f) {
  if (dtype == DG_BF16) return hist_dispatch_mode<QUAD, bf16_t>(mode, f);
  return hist_dispatch_mode<QUAD, float>(mode, f);
}

// ---- device loaders ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double hist_shfl_xor_f64(double v, int m) {
  return __longlong_as_double(__shfl_xor(__double_as_longlong(v), m, 64));
}

// all channels of a pixel loaded as 16 bytes (HIST_PIX16): 8 bf16, or 4 fp32 and zeros
template <typename T>
__device__ __forceinline__ void hist_unpack16(const uint4& r, float (&v)[HIST_MAXC]) {
  const unsigned u[4] = {r.x, r.y, r.z, r.w};
  if (sizeof(T) == 2) {
#pragma unroll
    for (int c = 0; c < HIST_MAXC; ++c) v[c] = __uint_as_float(c & 1 ? u[c / 2] & 0xffff0000u : u[c / 2] << 16);
  } else {
#pragma unroll
    for (int c = 0; c < HIST_MAXC; ++c) v[c] = c < 4 ? __uint_as_float(u[c & 3]) : 0.f;
  }
}

// channel c (wave-uniform) of such a pixel by selects: no register array to index
template <typename T>
__device__ __forceinline__ float hist_pick16_sel(const uint4& r, int c) {
  const int w = sizeof(T) == 2 ? c >> 1 : c;
  const unsigned word = w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w;
  if (sizeof(T) == 2) return __uint_as_float(c & 1 ? word & 0xffff0000u : word << 16);
  return __uint_as_float(word);
}

// the same by shifts of the two 64-bit halves (the unit loader below)
template <typename T>
__device__ __forceinline__ float hist_pick16_shift(const uint4& r, int c) {
  const unsigned long long lo = ((unsigned long long)r.y << 32) | r.x, hi = ((unsigned long long)r.w << 32) | r.z;
  if (sizeof(T) == 2) {
    const unsigned long long q = c < 4 ? lo : hi;
    return __uint_as_float((unsigned)(q >> (16 * (c & 3))) << 16);
  }
  const unsigned long long q = c < 2 ? lo : hi;                      // fp32: C <= 4 in this mode
  return __uint_as_float((unsigned)(q >> (32 * (c & 1))));
}

// One pixel, every output channel (fss.hip, objects.hip, distmap.hip, iscale.hip, deform.hip): the nout output values of the pixel whose
// channel 0 is at q; MODE is HIST_PIX16 or HIST_ANY.  y beyond nout is 0.  hist_pixel_values is hist_pixel_load, the loads alone,
// followed by hist_pixel_finish, everything after them: a kernel whose walk is a chain of load latencies (iscale.hip) issues the
// loads of several pixels before it finishes the first.
template <int MODE> struct HistPixelRaw { float v[HIST_MAXC]; };
template <> struct HistPixelRaw<HIST_PIX16> { uint4 r; };

template <typename T, int MODE>
__device__ __forceinline__ void hist_pixel_load(const HistXform& xf, const T* q, long long ld_c, HistPixelRaw<MODE>& raw) {
  if constexpr (MODE == HIST_PIX16) {
    raw.r = *reinterpret_cast<const uint4*>(q);
  } else {
#pragma unroll
    for (int c = 0; c < HIST_MAXC; ++c) raw.v[c] = c < xf.C ? ld_elem(q + c * ld_c) : 0.f;
  }
}

template <typename T, int MODE>
__device__ __forceinline__ void hist_pixel_finish(const HistXform& xf, const HistPixelRaw<MODE>& raw, float (&y)[HIST_MAXO]) {
  float v[HIST_MAXC];
  if constexpr (MODE == HIST_PIX16) {
    hist_unpack16<T>(raw.r, v);
  } else {
#pragma unroll
    for (int c = 0; c < HIST_MAXC; ++c) v[c] = raw.v[c];
  }
  float yu = 0.f, yv = 0.f;
#pragma unroll
  for (int c = 0; c < HIST_MAXC; ++c) {
    y[c] = hist_affine(v[c], xf.scale[c], xf.offset[c]);
    yu = c == xf.su ? y[c] : yu;
    yv = c == xf.sv ? y[c] : yv;
  }
  y[HIST_MAXO - 1] = 0.f;
  if (xf.speed) {
    const float s = hist_speed(yu, yv);
#pragma unroll
    for (int j = 0; j < HIST_MAXO; ++j) y[j] = j == xf.C ? s : y[j];
  }
}

template <typename T, int MODE>
__device__ __forceinline__ void hist_pixel_values(const HistXform& xf, const T* q, long long ld_c, float (&y)[HIST_MAXO]) {
  HistPixelRaw<MODE> raw;
  hist_pixel_load<T, MODE>(xf, q, ld_c, raw);
  hist_pixel_finish<T, MODE>(xf, raw, y);
}

// One item, every input channel, untransformed (histogram.hip, joint.hip): item i of field t is the pixel quad i in HIST_NCHW4
// (v[0 .. 3]), else the pixel i (v[0]).  Channels beyond C are left as they are, except in HIST_PIX16, which unpacks all 16 bytes.
template <typename T, int MODE>
__device__ __forceinline__ void hist_load_item(const HistSeries& s, int C, long long t, long long i, float (&v)[4][HIST_MAXC]) {
  const T* base = reinterpret_cast<const T*>(s.base);
  if (MODE == HIST_NCHW4) {
    const T* q = base + t * s.ld_t + 4 * i;
#pragma unroll
    for (int c = 0; c < HIST_MAXC; ++c) {
      if (c < C) {
        float w[4];
        ld4(q + c * s.ld_c, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k][c] = w[k];
      }
    }
  } else if (MODE == HIST_PIX16) {
    hist_unpack16<T>(*reinterpret_cast<const uint4*>(base + t * s.ld_t + i * s.ld_p), v[0]);
  } else {
    const T* q = base + t * s.ld_t + i * s.ld_p;
#pragma unroll
    for (int c = 0; c < HIST_MAXC; ++c)
      if (c < C) v[0][c] = ld_elem(q + c * s.ld_c);
  }
}

// Units (gridstats.hip, gridhist.hip): a thread keeps the running state of UNITS units, four pixels of one output channel
// (HIST_NCHW4) or one pixel of three.  HistUnit is what a unit reads: output channel j from the input channels c1 (and c2: the
// speed); a kernel's own unit struct derives from it and adds what it does with y, and the kernel fills its units in its loop over
// the groups of output channels (a shared helper for that made the compiler build that loop differently, at 1 - 3 VGPRs more).
struct HistUnit {
  int j, c1, c2;
  bool on, spd;
  float sc1, of1, sc2, of2;
};
template <int MODE, int UNITS> struct HistRaw { float x1[UNITS], x2[UNITS]; };
template <int UNITS> struct HistRaw<HIST_PIX16, UNITS> { uint4 r; };

// the loads of one field of one series for the UNITS units of this thread (i: pixel quad in HIST_NCHW4, else pixel)
template <typename T, int MODE, int UNITS, bool SPD, typename U>
__device__ __forceinline__ void hist_unit_load(const HistSeries& s, long long t, long long i, const U (&un)[UNITS], HistRaw<MODE, UNITS>& r) {
  const T* base = reinterpret_cast<const T*>(s.base);
  if constexpr (MODE == HIST_NCHW4) {
    const T* q = base + t * s.ld_t + 4 * i;
    ld4(q + un[0].c1 * s.ld_c, r.x1);
    if (SPD) ld4(q + un[0].c2 * s.ld_c, r.x2);
  } else if constexpr (MODE == HIST_PIX16) {
    r.r = *reinterpret_cast<const uint4*>(base + t * s.ld_t + i * s.ld_p);
  } else {
    const T* q = base + t * s.ld_t + i * s.ld_p;
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      r.x1[k] = ld_elem(q + un[k].c1 * s.ld_c);
      r.x2[k] = r.x1[k];
      if (un[k].spd) r.x2[k] = ld_elem(q + un[k].c2 * s.ld_c);       // wave-uniform
    }
  }
}

// the output value of unit k
template <typename T, int MODE, int UNITS, bool SPD>
__device__ __forceinline__ float hist_unit_value(const HistRaw<MODE, UNITS>& r, const HistUnit& un, int k) {
  float x1, x2;
  if constexpr (MODE == HIST_PIX16) {
    x1 = hist_pick16_shift<T>(r.r, un.c1);
    x2 = SPD ? hist_pick16_shift<T>(r.r, un.c2) : x1;
  } else {
    x1 = r.x1[k];
    x2 = MODE == HIST_NCHW4 && !SPD ? x1 : r.x2[k];
  }
  float y = hist_affine(x1, un.sc1, un.of1);
  if (SPD && un.spd) y = hist_speed(y, hist_affine(x2, un.sc2, un.of2));   // wave-uniform
  return y;
}
