// MXFP8 quantisation for the fp8 conv path (BASELINE.json configs[4]; reference math: DoWnGAN/networks/critic.py:20-88).
//
// Element format OCP FP8 E4M3 (gfx950's native fp8), one shared E8M0 scale (a power of two) per block of 32 CONSECUTIVE
// reduction channels (the OCP MX layout) -- the operand format of v_mfma_scale_f32_16x16x128_f8f6f4.  How the instruction
// maps registers to K (measured with tools/fp8_probe2.hip, not documented in the guides): lane (row r = l & 15, group
// g = l >> 4) holds 32 operand bytes; byte j is K index 64 * (j / 16) + 16 * g + (j % 16), and the scale of K block kb
// (= K / 32) of row r is byte `opsel` of the scale register of lane r + 16 * kb.  So a lane that loads the 16-byte chunk g of
// the first and of the second 64-byte half of a 128-channel row -- what the bf16 conv kernel's two fragment reads do -- feeds
// channels 16g.. and 64 + 16g.. in place, the four scale blocks are channels [0,32) [32,64) [64,96) [96,128) of the row, and
// lane (r, g) supplies the scale of block g.
// scale byte s: value 2^(s - 127); chosen as 2^(floor(log2(amax)) - 8) (8 = emax of E4M3, OCP MX rule); elements are
// x / scale rounded to nearest even, saturated at +-448.  A block that holds a NaN or an Inf becomes 32 x NaN (0x7F), so a
// non-finite activation or adjoint stays visible down the fp8 chain instead of being clamped into a finite value.
#include "dg_internal.h"

typedef __attribute__((ext_vector_type(4))) unsigned int q_u32x4_t;

template <typename T> struct QLoad;
template <> struct QLoad<bf16_t> {   // 16 channels = 32 bytes
  static __device__ __forceinline__ void run(const bf16_t* p, float* v) {
    const q_u32x4_t a = *reinterpret_cast<const q_u32x4_t*>(p), b = *reinterpret_cast<const q_u32x4_t*>(p + 8);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[2 * q] = __uint_as_float(a[q] << 16); v[2 * q + 1] = __uint_as_float(a[q] & 0xffff0000u);
      v[8 + 2 * q] = __uint_as_float(b[q] << 16); v[9 + 2 * q] = __uint_as_float(b[q] & 0xffff0000u);
    }
  }
};
template <> struct QLoad<float> {
  static __device__ __forceinline__ void run(const float* p, float* v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 t = reinterpret_cast<const float4*>(p)[q];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  }
};

// one thread = one block of one row: rows x (C / 32) threads
template <typename T>
__global__ void __launch_bounds__(256) quant_mxfp8_kernel(const T* __restrict__ src, long long rows, long long ld, int C,
                                                          unsigned char* __restrict__ q, long long ldq, unsigned char* __restrict__ sc,
                                                          long long ldqs) {
  dg_fp8_saturate_whole_kernel();
  const int nb = C >> 5;
  const long long total = rows * nb;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long r = t / nb;
    const int b = (int)(t - r * nb);
    const int c_lo = b * 32;
    float v[32];
    QLoad<T>::run(src + r * ld + c_lo, v);
    QLoad<T>::run(src + r * ld + c_lo + 16, v + 16);
    const unsigned a0 = mx_amax_bits16(v), a1 = mx_amax_bits16(v + 16);
    const unsigned ab = a0 > a1 ? a0 : a1;                       // a NaN / Inf anywhere in the block dominates
    const int e = mx_scale_byte(__uint_as_float(ab));
    const float inv = mx_inv_scale(e);
    *reinterpret_cast<q_u32x4_t*>(q + r * ldq + c_lo) = mx_poison(pack_fp8x16(v, inv), ab);
    *reinterpret_cast<q_u32x4_t*>(q + r * ldq + c_lo + 16) = mx_poison(pack_fp8x16(v + 16, inv), ab);
    sc[r * ldqs + b] = (unsigned char)e;
  }
}

extern "C" int dg_quant_mxfp8(int src_dtype, const void* src, int64_t rows, int64_t ld, int C, void* q, int64_t ldq, void* scales,
                              int64_t ldqs, void* stream) {
  if (ldqs <= 0) ldqs = C / 32;
  if (!src || !q || !scales || rows <= 0 || C <= 0 || C % 128 || ld < C || ldq < C || ldq % 16 || ldqs < C / 32) return DG_ERR_BAD_SHAPE;
  if ((src_dtype == DG_BF16 && ld % 8) || (src_dtype == DG_F32 && ld % 4)) return DG_ERR_BAD_SHAPE;
  const long long total = (long long)rows * (C / 32);
  long long nb = (total + 255) / 256;
  if (nb > 65536) nb = 65536;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (src_dtype == DG_BF16)
    hipLaunchKernelGGL(quant_mxfp8_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, (const bf16_t*)src, (long long)rows, (long long)ld, C,
                       (unsigned char*)q, (long long)ldq, (unsigned char*)scales, (long long)ldqs);
  else if (src_dtype == DG_F32)
    hipLaunchKernelGGL(quant_mxfp8_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, (const float*)src, (long long)rows, (long long)ld, C,
                       (unsigned char*)q, (long long)ldq, (unsigned char*)scales, (long long)ldqs);
  else return DG_ERR_BAD_DTYPE;
  return dg_check_launch();
}

// ---- per-block maximum of the MXFP8 scale bytes of up to DG_EXP_BATCH_MAX tensors (rows x nblocks bytes each) in ONE launch: the
// exponents of their uniform-scale copies.  blockIdx.y = tensor.  Threads walk dwords of the byte matrix (nblocks is a multiple of 4:
// channel counts are multiples of 128) with a running byte-wise maximum, reduce through LDS, then ONE atomicMax per block and
// workgroup into the caller's scratch (64 dwords per tensor, zero at rest: the finish kernel clears what it read).  (One atomic
// per THREAD -- 2 M atomics on <= 64 addresses per call -- cost the fp8 train step +40 ms.)
__global__ void __launch_bounds__(256) block_exp_max_kernel(const dg_exp_batch b, unsigned* __restrict__ tmp_all) {
  const int ti = blockIdx.y;
  const unsigned* __restrict__ sc = reinterpret_cast<const unsigned*>(b.scales[ti]);
  const long long rows = b.rows[ti], ld4 = b.ld[ti] / 4;
  const int nb4 = b.nblocks[ti] / 4;
  unsigned* tmp = tmp_all + ti * 64;
  const int col = threadIdx.x % nb4, sub = threadIdx.x / nb4, nsub = 256 / nb4;
  unsigned m = 0;
  for (long long r = (long long)blockIdx.x * nsub + sub; sub < nsub && r < rows; r += (long long)gridDim.x * nsub) {
    const unsigned v = sc[r * ld4 + col];
    unsigned r4 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const unsigned x = (v >> (8 * k)) & 0xffu, y = (m >> (8 * k)) & 0xffu; r4 |= (x > y ? x : y) << (8 * k); }
    m = r4;
  }
  __shared__ unsigned sm[256];
  sm[threadIdx.x] = m;
  __syncthreads();
  if ((int)threadIdx.x < nb4) {
    unsigned r4 = 0;
    for (int k = 0; k < nsub; ++k) {
      const unsigned v = sm[k * nb4 + threadIdx.x];
#pragma unroll
      for (int q = 0; q < 4; ++q) { const unsigned x = (v >> (8 * q)) & 0xffu, y = (r4 >> (8 * q)) & 0xffu; r4 = (r4 & ~(0xffu << (8 * q))) | ((x > y ? x : y) << (8 * q)); }
    }
    if (r4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) atomicMax(tmp + threadIdx.x * 4 + q, (r4 >> (8 * q)) & 0xffu);
    }
  }
}
__global__ void block_exp_finish_kernel(const dg_exp_batch b, unsigned* __restrict__ tmp_all, int margin) {
  const int ti = blockIdx.x, k = threadIdx.x;
  unsigned* tmp = tmp_all + ti * 64;
  if (k < b.nblocks[ti]) {
    unsigned v = tmp[k] + (unsigned)margin;
    // passes over one buffer alternate between inputs of different size (real / generated samples: 20x apart at initialisation), and
    // exponents taken from the smaller one saturate the larger one's copy at 448 * 2^e: an exponent falls by at most ONE per update
    const unsigned old = reinterpret_cast<unsigned char*>(b.out[ti])[k];
    if (old > 0u && v + 1u < old) v = old - 1u;
    reinterpret_cast<unsigned char*>(b.out[ti])[k] = (unsigned char)(v > 254u ? 254u : v);
    tmp[k] = 0u;
  }
}

extern "C" int dg_block_exp_max_batch(const dg_exp_batch* b, int margin, void* scratch, void* stream) {
  if (!b || !scratch) return DG_ERR_BAD_ARG;
  if (b->n <= 0 || b->n > DG_EXP_BATCH_MAX || margin < 0 || margin > 8 || reinterpret_cast<uintptr_t>(scratch) % 4) return DG_ERR_BAD_SHAPE;
  long long maxwg = 1;
  for (int i = 0; i < b->n; ++i) {
    if (!b->scales[i] || !b->out[i]) return DG_ERR_BAD_ARG;
    const int nb = b->nblocks[i];
    if (b->rows[i] <= 0 || nb <= 0 || nb > 64 || nb % 4 || b->ld[i] < nb || b->ld[i] % 4 || reinterpret_cast<uintptr_t>(b->scales[i]) % 4) return DG_ERR_BAD_SHAPE;
    const long long nsub = 256 / (nb / 4);
    long long nwg = (b->rows[i] + nsub * 64 - 1) / (nsub * 64);
    if (nwg > maxwg) maxwg = nwg;
  }
  if (maxwg > 512) maxwg = 512;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(block_exp_max_kernel, dim3((unsigned)maxwg, (unsigned)b->n), dim3(256), 0, st, *b, (unsigned*)scratch);
  hipLaunchKernelGGL(block_exp_finish_kernel, dim3((unsigned)b->n), dim3(64), 0, st, *b, (unsigned*)scratch, margin);
  return dg_check_launch();
}

extern "C" int dg_block_exp_max(const void* scales, int64_t rows, int64_t ld, int nblocks, int margin, void* out, void* scratch, void* stream) {
  dg_exp_batch b{};
  b.n = 1; b.scales[0] = scales; b.rows[0] = rows; b.ld[0] = ld; b.nblocks[0] = nblocks; b.out[0] = out;
  return dg_block_exp_max_batch(&b, margin, scratch, stream);
}

// dg_epilogue.out_amax -> exponents: out[b] = min(254, mx_scale_byte(largest magnitude of block b) + margin) -- what dg_block_exp_max gives
// for the MXFP8 scale bytes of the same tensor (the largest per-pixel block exponent IS the exponent of the largest value) -- and the
// census is cleared for the next pass.
__global__ void exp_from_amax_kernel(unsigned* __restrict__ amax, int nblocks, int margin, unsigned char* __restrict__ out) {
  const int k = threadIdx.x;
  if (k < nblocks) {
    unsigned v = (unsigned)mx_scale_byte(__uint_as_float(amax[k])) + (unsigned)margin;
    const unsigned old = out[k];
    if (old > 0u && v + 1u < old) v = old - 1u;       // (falls by at most one per update, as in block_exp_finish_kernel)
    out[k] = (unsigned char)(v > 254u ? 254u : v);
    amax[k] = 0u;
  }
}
extern "C" int dg_exp_from_amax(void* amax, int nblocks, int margin, void* out, void* stream) {
  if (!amax || !out) return DG_ERR_BAD_ARG;
  if (nblocks <= 0 || nblocks > 64 || margin < 0 || margin > 8 || reinterpret_cast<uintptr_t>(amax) % 4) return DG_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(exp_from_amax_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), (unsigned*)amax, nblocks, margin, (unsigned char*)out);
  return dg_check_launch();
}

// ---- stand-alone uniform-scale quantiser (the conv epilogues write this form themselves, dg_epilogue.out_u; this is for the one
// adjoint that does not come out of a conv: the FC's input gradient): q[r][c] = E4M3(src[r][c] / 2^(exps[c / 32] - 127)), a block
// that holds a NaN / Inf poisoned like the MXFP8 copy.  One thread = one 32-channel block of one row.
// The exponent here is the CALLER's, not one derived from the block: any byte 0 .. 254 against any finite value.  The one fp32 multiply
// of pack_fp8x16 does not cover that: 2^(127 - 254) is no normal fp32 number (mx_inv_scale(254) is the bit pattern of 0.0f: zeros were
// written), and a product past fp32's range (exponent field of v >= e + 128: |v| >= 4 under the byte 1 an all-zero block gets at
// margin 1) is Inf, which the converter keeps as NaN under FP16_OVFL -- 0x7F for a finite value, in a block that is not poisoned.
// v_ldexp_f32 scales exactly over the whole range and the clamp turns the Inf of an overflow into +-448, as the fused copy
// (pack_fp8x16_from_bf16) and the emulation's clamp do; a NaN / Inf SOURCE poisons its block afterwards (mx_poison).  Two VALU
// operations per value more than the multiply: this kernel is off the hot path (the FC's input gradient, one adjoint slice per RRDB).
__device__ __forceinline__ dg_u32x4_t pack_fp8x16_any_exp(const float* v, int e) {
  float t[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) t[k] = __builtin_amdgcn_fmed3f(__builtin_ldexpf(v[k], 127 - e), -448.f, 448.f);
  return pack_fp8x16(t, 1.f);
}

template <typename T>
__global__ void __launch_bounds__(256) quant_uniform_kernel(const T* __restrict__ src, long long rows, long long ld, int C,
                                                            const unsigned char* __restrict__ exps, unsigned char* __restrict__ q, long long ldq) {
  dg_fp8_saturate_whole_kernel();
  const int nb = C >> 5;
  const long long total = rows * nb;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long r = t / nb;
    const int b = (int)(t - r * nb);
    float v[32];
    QLoad<T>::run(src + r * ld + b * 32, v);
    QLoad<T>::run(src + r * ld + b * 32 + 16, v + 16);
    const unsigned a0 = mx_amax_bits16(v), a1 = mx_amax_bits16(v + 16);
    const unsigned ab = a0 > a1 ? a0 : a1;
    const int e = (int)exps[b];
    *reinterpret_cast<q_u32x4_t*>(q + r * ldq + b * 32) = mx_poison(pack_fp8x16_any_exp(v, e), ab);
    *reinterpret_cast<q_u32x4_t*>(q + r * ldq + b * 32 + 16) = mx_poison(pack_fp8x16_any_exp(v + 16, e), ab);
  }
}

extern "C" int dg_quant_uniform(int src_dtype, const void* src, int64_t rows, int64_t ld, int C, const void* exps, void* q, int64_t ldq,
                                void* stream) {
  if (!src || !q || !exps) return DG_ERR_BAD_ARG;
  if (rows <= 0 || C <= 0 || C % 128 || ld < C || ldq < C || ldq % 16) return DG_ERR_BAD_SHAPE;
  if ((src_dtype == DG_BF16 && ld % 8) || (src_dtype == DG_F32 && ld % 4)) return DG_ERR_BAD_SHAPE;
  const long long total = (long long)rows * (C / 32);
  long long nb = (total + 255) / 256;
  if (nb > 65536) nb = 65536;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (src_dtype == DG_BF16)
    hipLaunchKernelGGL(quant_uniform_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, (const bf16_t*)src, (long long)rows, (long long)ld, C,
                       (const unsigned char*)exps, (unsigned char*)q, (long long)ldq);
  else if (src_dtype == DG_F32)
    hipLaunchKernelGGL(quant_uniform_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, (const float*)src, (long long)rows, (long long)ld, C,
                       (const unsigned char*)exps, (unsigned char*)q, (long long)ldq);
  else return DG_ERR_BAD_DTYPE;
  return dg_check_launch();
}
