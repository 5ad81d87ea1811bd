// The value transform and the load-mode rule shared by the value histograms (histogram.hip) and the per-gridpoint statistics
// (gridstats.hip): both read fields through dg_eof_fields and must see the same output values y bit for bit.
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
