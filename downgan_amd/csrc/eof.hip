// EOF analysis (include/downgan_hip.h "EOF analysis"): per-channel PCA of a time series of fields.
//   eof_mean_kernel          mu[c][p] = mean_t x[t,c,p]                                   (fp64 accumulation)
//   eof_xyt_kernel           split-P  S[i][j] = sum_p (a[i,c,p] - ma[c,p]) (b[j,c,p] - mb[c,p]) on v_mfma_f32_32x32x2_f32,
//                            one 64 x 64 tile of every channel per workgroup, written as an fp32 partial slab per P slice:
//                            the centred Gram (a = b = x, upper-triangle tiles) and the projection (a = y, b = E)
//   eof_reduce_kernel        slabs of one tile summed over the slices in a fixed order (fp64) -> G (mirrored) or Z
//   eof_components_kernel    E[c][k][p] = sum_t A[c][t][k] (x[t,c,p] - mu[c,p]) + the position of each row's largest |entry|
//   eof_sign_kernel / eof_flip_kernel   sklearn's sign rule applied in place
//   eof_reconstruct_kernel   out[b][c][p] = sum_k Z[b][c][k] E[c][k][p] (+ mu)
// Nothing here uses float atomics: every sum runs in a fixed order, so repeated calls are bit-identical.  The only atomic is
// the integer max of the components' position keys, whose result does not depend on the order.
#include "dg_internal.h"

namespace {

template <typename T>
__device__ __forceinline__ const T* elem_ptr(const void* base, long long off) { return reinterpret_cast<const T*>(base) + off; }

// ---------------------------------------------------------------------------------------------------------------- mean
// one thread per (c, p); consecutive workgroups take the channels of one pixel range, so an interleaved ([n, H, W, c]) store is
// fetched from HBM once and its other channels hit in L2
template <typename T>
__global__ __launch_bounds__(256) void eof_mean_kernel(const T* x, int Tn, int C, int P, long long ld_t, long long ld_c,
                                                       long long ld_p, float* mu) {
  const int c = blockIdx.x % C;
  const long long p = (long long)(blockIdx.x / C) * 256 + threadIdx.x;
  if (p >= P) return;
  const T* q = x + c * ld_c + p * ld_p;
  double s = 0.0;
#pragma unroll 8
  for (int t = 0; t < Tn; ++t) s += (double)ld_elem(q + (long long)t * ld_t);
  mu[(long long)c * P + p] = (float)(s / Tn);
}

// ---------------------------------------------------------------------------------------------------------- x . y^T
struct EofSide {
  const void* base;
  const float* mean;      // [C][P] or NULL
  long long ld_t, ld_c, ld_p;
  int rows;
};
struct EofXY {
  EofSide a, b;
  int P, upper, nta, ntb, ntiles;
  long long slice_len;    // pixels per slice, a multiple of 64
  float* ws;              // [nslice][ntiles][NC][64][64]
};

// pixels per chunk: KP * NC = 64 columns (c, p) of one staged chunk
template <int NC> struct EofKP { static constexpr int v = NC == 1 ? 64 : NC == 2 ? 32 : NC <= 4 ? 16 : 8; };

__device__ __forceinline__ void eof_tile(int tile, int upper, int nta, int ntb, int& ti, int& tj) {
  if (upper) {
    int t = tile;
    ti = 0;
    while (t >= nta - ti) { t -= nta - ti; ++ti; }
    tj = ti + t;
  } else {
    ti = tile / ntb;
    tj = tile % ntb;
  }
}

// lane -> (channel, pixel) column of a chunk; pixel-major when the channels are interleaved, so the 64 lanes of a row load
// contiguous elements in either layout
template <int NC, int KP>
__device__ __forceinline__ void eof_column(const EofSide& s, int lane, int& c, int& p) {
  if (s.ld_c < s.ld_p) { p = lane / NC; c = lane % NC; }
  else { c = lane / KP; p = lane % KP; }
}

template <typename T, int NC, int KP>
__device__ __forceinline__ void eof_load_side(const EofSide& s, int c, int pc, int lane, int w, int row0, long long p0,
                                              long long p_end, int P, float* r) {
  const long long p = p0 + pc;
  const bool col_ok = lane < KP * NC && p < p_end;
  const float m = (col_ok && s.mean) ? s.mean[(long long)c * P + p] : 0.f;
  const T* q = elem_ptr<T>(s.base, col_ok ? c * s.ld_c + p * s.ld_p : 0);
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int row = row0 + w + 4 * it;
    r[it] = (col_ok && row < s.rows) ? ld_elem(q + (long long)row * s.ld_t) - m : 0.f;
  }
}

template <typename TA, typename TB, int NC>
__global__ __launch_bounds__(256) void eof_xyt_kernel(EofXY g) {
  constexpr int KP = EofKP<NC>::v, Q = KP * NC, LDR = 65;   // odd row pitch: the column-wise stores are bank-conflict free
  __shared__ float lds[2][Q][LDR];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wi = w >> 1, wj = w & 1;
  const int tile = blockIdx.x % g.ntiles, slice = blockIdx.x / g.ntiles;
  int ti, tj;
  eof_tile(tile, g.upper, g.nta, g.ntb, ti, tj);
  const long long p_begin = (long long)slice * g.slice_len;
  const long long p_end = p_begin + g.slice_len < g.P ? p_begin + g.slice_len : g.P;
  int ca, pa, cb, pb;
  eof_column<NC, KP>(g.a, lane, ca, pa);
  eof_column<NC, KP>(g.b, lane, cb, pb);
  const int qa = ca * KP + pa, qb = cb * KP + pb;   // LDS column, channel-major

  float ra[16], rb[16];
  // two-level fp32 sums: the MFMA chain covers EOF_SUB pixels, then folds into tot (up to 4 channels: the registers of 8 do not
  // fit twice; the host gives wider inputs shorter slices instead).  A chain of L fp32 fmas errs by ~L ulps of the running sum.
  constexpr bool TWO = NC <= 4;
  constexpr int EOF_SUB = 512;
  f32x16_t acc[NC], tot[TWO ? NC : 1];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;
#pragma unroll
  for (int c = 0; c < (TWO ? NC : 1); ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) tot[c][e] = 0.f;

  if (p_begin < p_end) {
    eof_load_side<TA, NC, KP>(g.a, ca, pa, lane, w, ti * 64, p_begin, p_end, g.P, ra);
    eof_load_side<TB, NC, KP>(g.b, cb, pb, lane, w, tj * 64, p_begin, p_end, g.P, rb);
  }
  for (long long p0 = p_begin; p0 < p_end; p0 += KP) {
    __syncthreads();                        // the previous chunk's fragment reads are done
    if (lane < Q) {
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        lds[0][qa][w + 4 * it] = ra[it];
        lds[1][qb][w + 4 * it] = rb[it];
      }
    }
    __syncthreads();
    if (p0 + KP < p_end) {                  // next chunk in flight behind this chunk's MFMAs
      eof_load_side<TA, NC, KP>(g.a, ca, pa, lane, w, ti * 64, p0 + KP, p_end, g.P, ra);
      eof_load_side<TB, NC, KP>(g.b, cb, pb, lane, w, tj * 64, p0 + KP, p_end, g.P, rb);
    }
    // v_mfma_f32_32x32x2_f32: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
#pragma unroll
    for (int s = 0; s < KP / 2; ++s) {
      const int kp = 2 * s + (lane >> 5);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float av = lds[0][c * KP + kp][wi * 32 + (lane & 31)];
        const float bv = lds[1][c * KP + kp][wj * 32 + (lane & 31)];
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[c], 0, 0, 0);
      }
    }
    if (TWO && (p0 + KP - p_begin) % EOF_SUB == 0) {
#pragma unroll
      for (int c = 0; c < (TWO ? NC : 1); ++c) {
        tot[c] += acc[c];
        acc[c] = f32x16_t{};
      }
    }
  }
  if (TWO) {
#pragma unroll
    for (int c = 0; c < (TWO ? NC : 1); ++c) acc[c] += tot[c];
  }
  // C/D map: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  float* slab = g.ws + (long long)blockIdx.x * NC * 4096;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
      slab[c * 4096 + (wi * 32 + row) * 64 + wj * 32 + (lane & 31)] = acc[c][e];
    }
}

// one thread per (tile, c, element): the nslice partials in slice order, in fp64
__global__ __launch_bounds__(256) void eof_reduce_kernel(const float* ws, int nslice, int ntiles, int NC, int upper, int nta,
                                                         int ntb, int Ta, int Tb, double* G, float* Z) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)ntiles * NC * 4096) return;
  const int e = (int)(idx & 4095), c = (int)((idx >> 12) % NC), tile = (int)((idx >> 12) / NC);
  int ti, tj;
  eof_tile(tile, upper, nta, ntb, ti, tj);
  const int I = ti * 64 + (e >> 6), J = tj * 64 + (e & 63);
  if (I >= Ta || J >= Tb || (upper && I > J)) return;
  double s = 0.0;
  const long long stride = (long long)ntiles * NC * 4096;
  const float* q = ws + idx;
  for (int sl = 0; sl < nslice; ++sl) s += (double)q[sl * stride];
  if (G) {
    G[((long long)c * Ta + I) * Ta + J] = s;
    G[((long long)c * Ta + J) * Ta + I] = s;
  } else {
    Z[((long long)I * NC + c) * Tb + J] = (float)s;
  }
}

// --------------------------------------------------------------------------------------------------------- components
template <typename T, int KB>
__global__ __launch_bounds__(256) void eof_components_kernel(const T* x, int Tn, int C, int P, long long ld_t, long long ld_c,
                                                             long long ld_p, const float* mu, const float* A, int K,
                                                             float* E, long long ld_k, long long ld_ce,
                                                             unsigned long long* amax) {
  __shared__ unsigned long long red[4][KB];
  const int c = blockIdx.x % C;
  const long long p = (long long)(blockIdx.x / C) * 256 + threadIdx.x;
  const bool ok = p < P;
  const long long pl = ok ? p : P - 1;    // out-of-range lanes compute a duplicate and store nothing: no divergent loop
  const T* q = x + c * ld_c + pl * ld_p;
  const float m = mu[(long long)c * P + pl];
  const float* a = A + (long long)c * Tn * KB;   // uniform over the workgroup: scalar loads
  float acc[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) acc[k] = 0.f;
  for (int t = 0; t < Tn; ++t) {
    const float v = ld_elem(q + (long long)t * ld_t) - m;
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = fmaf(a[(long long)t * KB + k], v, acc[k]);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    if (k < K && ok) E[c * ld_ce + k * ld_k + p] = acc[k];
    // key: |value| bits above, (0xffffffff - p) below -> the integer max is the largest magnitude, ties to the lowest p
    unsigned long long key = ok ? (((unsigned long long)__float_as_uint(fabsf(acc[k])) << 32) | (0xffffffffu - (unsigned)p)) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o, 64);
      key = other > key ? other : key;
    }
    if (lane == 0) red[w][k] = key;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    unsigned long long key = red[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < 4; ++i) key = red[i][threadIdx.x] > key ? red[i][threadIdx.x] : key;
    atomicMax(amax + (long long)c * K + threadIdx.x, key);
  }
}

// bit 63 of a key (the sign bit of |value|, always clear) := "the entry at the key's position is negative"
__global__ void eof_sign_kernel(const float* E, int C, int K, long long ld_k, long long ld_ce, unsigned long long* amax) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= C * K) return;
  const int c = i / K, k = i % K;
  const unsigned long long key = amax[i] & ~(1ull << 63);
  if (key == 0) { amax[i] = 0; return; }
  const unsigned p = 0xffffffffu - (unsigned)(key & 0xffffffffu);
  const bool neg = E[c * ld_ce + k * ld_k + p] < 0.f;
  amax[i] = key | ((unsigned long long)neg << 63);
}

__global__ __launch_bounds__(256) void eof_flip_kernel(float* E, int K, int P, long long ld_k, long long ld_ce,
                                                       const unsigned long long* amax) {
  const int ck = blockIdx.y, c = ck / K, k = ck % K;
  if (!(amax[ck] >> 63)) return;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < P) {
    float* e = E + c * ld_ce + k * ld_k + p;
    *e = -*e;
  }
}

// ------------------------------------------------------------------------------------------------------- reconstruct
template <int KB>
__global__ __launch_bounds__(256) void eof_reconstruct_kernel(const float* Z, int B, int C, int K, const float* E, long long ld_k,
                                                              long long ld_ce, int P, const float* mu, float* out) {
  const int c = blockIdx.x % C;
  const long long p = (long long)(blockIdx.x / C) * 256 + threadIdx.x;
  if (p >= P) return;
  float e[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) e[k] = k < K ? E[c * ld_ce + k * ld_k + p] : 0.f;
  const float m = mu ? mu[(long long)c * P + p] : 0.f;
  for (int b = 0; b < B; ++b) {
    const float* z = Z + ((long long)b * C + c) * K;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (k < K) s = fmaf(z[k], e[k], s);
    out[((long long)b * C + c) * P + p] = s + m;
  }
}

// -------------------------------------------------------------------------------------------------------------- host
bool fields_ok(const dg_eof_fields* x) {
  return x && x->base && x->T >= 1 && x->C >= 1 && x->C <= DG_EOF_MAX_C && x->P >= 1 && x->ld_t >= 0 && x->ld_c >= 0 &&
         x->ld_p >= 0;
}

EofSide side_of(const dg_eof_fields* x, const float* mean) {
  EofSide s;
  s.base = x->base; s.mean = mean; s.ld_t = x->ld_t; s.ld_c = x->ld_c; s.ld_p = x->ld_p; s.rows = x->T;
  return s;
}

template <typename TA, typename TB>
int launch_xyt_t(const EofXY& g, int NC, unsigned blocks, hipStream_t st) {
  switch (NC) {
#define DG_EOF_NC(n) case n: hipLaunchKernelGGL((eof_xyt_kernel<TA, TB, n>), dim3(blocks), dim3(256), 0, st, g); break;
    DG_EOF_NC(1) DG_EOF_NC(2) DG_EOF_NC(3) DG_EOF_NC(4) DG_EOF_NC(5) DG_EOF_NC(6) DG_EOF_NC(7) DG_EOF_NC(8)
#undef DG_EOF_NC
    default: return DG_ERR_BAD_SHAPE;
  }
  return DG_OK;
}

// S = a . b^T over nslice P slices into ws, then the ordered slice sum into G (fp64, mirrored) or Z
int launch_xyt(EofXY g, int dta, int dtb, int NC, int nslice, double* G, float* Z, hipStream_t st) {
  const long long ceil64 = ((long long)g.P + 63) / 64;
  if (nslice < 1 || nslice > ceil64) return DG_ERR_BAD_SHAPE;
  g.slice_len = (ceil64 + nslice - 1) / nslice * 64;
  const long long blocks = (long long)nslice * g.ntiles;
  if (blocks > 0x7fffffffLL) return DG_ERR_BAD_SHAPE;
  int rc;
  if (dta == DG_F32 && dtb == DG_F32) rc = launch_xyt_t<float, float>(g, NC, (unsigned)blocks, st);
  else if (dta == DG_BF16 && dtb == DG_BF16) rc = launch_xyt_t<bf16_t, bf16_t>(g, NC, (unsigned)blocks, st);
  else if (dta == DG_BF16 && dtb == DG_F32) rc = launch_xyt_t<bf16_t, float>(g, NC, (unsigned)blocks, st);
  else return DG_ERR_BAD_DTYPE;
  if (rc != DG_OK) return rc;
  const long long n = (long long)g.ntiles * NC * 4096;
  hipLaunchKernelGGL(eof_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)g.ws, nslice,
                     g.ntiles, NC, g.upper, g.nta, g.ntb, g.a.rows, g.b.rows, G, Z);
  return dg_check_launch();
}

}  // namespace

extern "C" int dg_eof_mean(const dg_eof_fields* x, float* mu, void* stream) {
  if (!fields_ok(x) || !mu) return DG_ERR_BAD_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long long blocks = (long long)x->C * ((x->P + 255) / 256);
  if (x->dtype == DG_F32)
    hipLaunchKernelGGL(eof_mean_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)x->base, x->T, x->C, x->P,
                       (long long)x->ld_t, (long long)x->ld_c, (long long)x->ld_p, mu);
  else if (x->dtype == DG_BF16)
    hipLaunchKernelGGL(eof_mean_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)x->base, x->T, x->C, x->P,
                       (long long)x->ld_t, (long long)x->ld_c, (long long)x->ld_p, mu);
  else return DG_ERR_BAD_DTYPE;
  return dg_check_launch();
}

extern "C" int dg_eof_gram(const dg_eof_fields* x, const float* mu, int nslice, float* ws, double* G, void* stream) {
  if (!fields_ok(x) || !mu || !ws || !G) return DG_ERR_BAD_SHAPE;
  EofXY g;
  g.a = side_of(x, mu); g.b = g.a;
  g.P = x->P; g.upper = 1;
  g.nta = g.ntb = (x->T + 63) / 64;
  g.ntiles = g.nta * (g.nta + 1) / 2;
  g.ws = ws;
  return launch_xyt(g, x->dtype, x->dtype, x->C, nslice, G, nullptr, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dg_eof_project(const dg_eof_fields* y, const float* m, const float* E, int K, int64_t ld_k, int64_t ld_c, int nslice,
                              float* ws, float* Z, void* stream) {
  if (!fields_ok(y) || !E || !ws || !Z || K < 1 || K > DG_EOF_MAX_K || ld_k < 0 || ld_c < 0) return DG_ERR_BAD_SHAPE;
  EofXY g;
  g.a = side_of(y, m);
  g.b.base = E; g.b.mean = nullptr; g.b.ld_t = ld_k; g.b.ld_c = ld_c; g.b.ld_p = 1; g.b.rows = K;
  g.P = y->P; g.upper = 0;
  g.nta = (y->T + 63) / 64; g.ntb = 1;
  g.ntiles = g.nta;
  g.ws = ws;
  return launch_xyt(g, y->dtype, DG_F32, y->C, nslice, nullptr, Z, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dg_eof_components(const dg_eof_fields* x, const float* mu, const float* A, int K, float* E, int64_t ld_k,
                                 int64_t ld_c, unsigned long long* amax, void* stream) {
  if (!fields_ok(x) || !mu || !A || !E || !amax || K < 1 || K > DG_EOF_MAX_K || ld_k < 0 || ld_c < 0) return DG_ERR_BAD_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)((long long)x->C * ((x->P + 255) / 256));
  const int KB = (K + 15) / 16 * 16;
#define DG_EOF_COMP(TY, kb)                                                                                                      \
  hipLaunchKernelGGL((eof_components_kernel<TY, kb>), dim3(blocks), dim3(256), 0, st, (const TY*)x->base, x->T, x->C, x->P,    \
                     (long long)x->ld_t, (long long)x->ld_c, (long long)x->ld_p, mu, A, K, E, (long long)ld_k, (long long)ld_c, amax)
#define DG_EOF_COMP_KB(TY)                                                                                                       \
  switch (KB) {                                                                                                                 \
    case 16: DG_EOF_COMP(TY, 16); break;                                                                                         \
    case 32: DG_EOF_COMP(TY, 32); break;                                                                                         \
    case 48: DG_EOF_COMP(TY, 48); break;                                                                                         \
    default: DG_EOF_COMP(TY, 64); break;                                                                                         \
  }
  if (x->dtype == DG_F32) { DG_EOF_COMP_KB(float) }
  else if (x->dtype == DG_BF16) { DG_EOF_COMP_KB(bf16_t) }
  else return DG_ERR_BAD_DTYPE;
#undef DG_EOF_COMP_KB
#undef DG_EOF_COMP
  return dg_check_launch();
}

extern "C" int dg_eof_flip(float* E, int C, int K, int P, int64_t ld_k, int64_t ld_c, const unsigned long long* amax, void* stream) {
  if (!E || !amax || C < 1 || C > DG_EOF_MAX_C || K < 1 || K > DG_EOF_MAX_K || P < 1 || ld_k < 0 || ld_c < 0) return DG_ERR_BAD_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(eof_sign_kernel, dim3((C * K + 63) / 64), dim3(64), 0, st, (const float*)E, C, K, (long long)ld_k, (long long)ld_c,
                     const_cast<unsigned long long*>(amax));
  hipLaunchKernelGGL(eof_flip_kernel, dim3((unsigned)((P + 255) / 256), C * K), dim3(256), 0, st, E, K, P, (long long)ld_k,
                     (long long)ld_c, amax);
  return dg_check_launch();
}

extern "C" int dg_eof_reconstruct(const float* Z, int B, int C, int K, const float* E, int64_t ld_k, int64_t ld_c, int P,
                                  const float* mu, float* out, void* stream) {
  if (!Z || !E || !out || B < 1 || C < 1 || C > DG_EOF_MAX_C || K < 1 || K > DG_EOF_MAX_K || P < 1 || ld_k < 0 || ld_c < 0)
    return DG_ERR_BAD_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)((long long)C * ((P + 255) / 256));
  const int KB = (K + 15) / 16 * 16;
#define DG_EOF_REC(kb) hipLaunchKernelGGL(eof_reconstruct_kernel<kb>, dim3(blocks), dim3(256), 0, st, Z, B, C, K, E, (long long)ld_k, \
                                          (long long)ld_c, P, mu, out)
  switch (KB) {
    case 16: DG_EOF_REC(16); break;
    case 32: DG_EOF_REC(32); break;
    case 48: DG_EOF_REC(48); break;
    default: DG_EOF_REC(64); break;
  }
#undef DG_EOF_REC
  return dg_check_launch();
}
