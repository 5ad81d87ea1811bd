// The value transform, the bin rules and the load-mode rule shared by the value histograms (histogram.hip), the per-gridpoint
// statistics (gridstats.hip), the joint histograms (joint.hip) and the increment histograms (increments.hip): all read fields
// through dg_eof_fields and must see the same output values y bit for bit.
#pragma once
#include <stdint.h>

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
