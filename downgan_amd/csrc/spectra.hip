// Radially averaged power spectra (include/downgan_hip.h "Radially averaged power spectra") of square N x N fields,
// N a power of two in [16, DG_RAPSD_MAX_N], read through the EOF field descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16).
//   rapsd_twiddle_kernel   tw[m] = exp(-2 pi i m / N), from double sincospi, rounded to fp32 once
//   rapsd_count_kernel     ring pixel counts (the same integer ring test as the host's dg_rapsd_ring_counts)
//   rapsd_row_kernel       two real rows packed as one complex N-point FFT (Stockham radix-4, radix-2 last stage when log2 N
//                          is odd, in LDS), split into the two half spectra u = 0..N/2, written transposed: spec[f][u][h]
//   rapsd_col_kernel       per line u of a field: complex N-point FFT along h, |X|^2 / N^2 with the Hermitian weight (1 for
//                          u = 0 and u = N/2, 2 otherwise), ring sums per workgroup (a slice of the lines) in fp64
//   rapsd_field_kernel     slices summed in a fixed order (fp64), divided by the ring counts -> per-field spectra
//   rapsd_sum_kernel       sum[c][k] = sum over t of the per-field spectra, in t order
// Ring k holds the frequencies (u, v) (signed, |u|, |v| <= N/2) with (2k-1)^2 <= 4 (u^2 + v^2) < (2k+1)^2, evaluated in integers:
// r^2 in [k^2 - k + 1, k^2 + k] (k = 0: r^2 = 0).  Rings k > N/2 (the corners) are dropped.  No float atomics anywhere: two
// calls on the same data are bit-identical.
//
// Cross spectra (include/downgan_hip.h "Cross spectra") of paired fields a, b: ring means of |A|^2 / N^2, |B|^2 / N^2 and
// Re(A conj B) / N^2 over the same rings.
//   rapsd_row_kernel       unchanged, once per side, into two half-spectrum buffers (each side has its own layout and dtype)
//   cross_col_kernel       per slice of lines u of a pair: FFT of side a's lines (kept in a third LDS buffer), FFT of side b's
//                          lines, the three weighted products per point, ring sums of each plane in fp64; the slices, the loop
//                          order and the power expression are those of rapsd_col_kernel, so planes 0 and 1 equal dg_rapsd of a
//                          and of b bit for bit.  LDS: 3 x 16 KB line buffers + 16 KB twiddles = 64 KB per workgroup, so two
//                          workgroups (8 waves) share a CU's 160 KB; rapsd_col_kernel's 48 KB would admit three.
//   cross_field_kernel     slices summed in order, divided by the ring counts -> per-field [3][K]
//   cross_sum_kernel       sum[c][plane][k] over t, in t order
//
// Helmholtz spectra (include/downgan_hip.h "Helmholtz spectra") of a vector field (u, v), U = su FFT2(u), V = sv FFT2(v): ring
// means of ke = (|U|^2 + |V|^2) / (2 N^2), rot = |kx V - ky U|^2 / (2 k2 N^2) and div = |kx U + ky V|^2 / (2 k2 N^2), kx the
// signed wavenumber along W (the line index u of the half spectra), ky along H, k2 = kx^2 + ky^2 (rot = div = 0 at k2 = 0); for
// a pair of vector fields also co_rot = Re(Ra conj Rb) / (2 k2 N^2) and co_div likewise, R = kx V - ky U, D = kx U + ky V.
//   rapsd_row_kernel       unchanged, once per component and side through a one-channel descriptor
//   helm_col_kernel        per slice of lines: helm_side (FFT of U^'s lines, parked in the third LDS buffer, FFT of V^'s lines,
//                          then per point in fp32 the scaled U, V and ke, rot, div with the Hermitian weight), the three planes
//                          ring-summed in fp64 with rapsd_col_kernel's slices and loop order.  LDS 64 KB as cross_col_kernel.
//   helm_cross_col_kernel  side a as above; its U, V stay in registers while side b runs through the same buffers; then side
//                          b's planes and the two co-planes.  Both kernels call the same helm_side and the same per-plane ring
//                          sums, so planes 0-5 equal the one-sided calls on a and on b bit for bit, and (a, a) gives
//                          co_rot = rot, co_div = div bit for bit.
//   helm_field_kernel, helm_sum_kernel   cross_field_kernel / cross_sum_kernel for 3 or 8 planes of one field per time
// NYQUIST RULE.  The half spectrum holds each conjugate pair once with weight 2.  At v = N/2 on a line 0 < u < N/2 the two
// members are (kx, -N/2) and (-kx, -N/2) in fftfreq's convention, and on the line u = N/2 the members (-N/2, v), (-N/2, -v) lie
// in one ring: in both cases the cross term 2 kx ky Re(U conj V) of |D|^2 and |R|^2 has opposite signs for the two and cancels
// in the ring sum.  So every point with u = N/2 or v = N/2 contributes WITHOUT the cross term,
//   div ~ kx^2 |U|^2 + ky^2 |V|^2,  rot ~ kx^2 |V|^2 + ky^2 |U|^2   (co-planes: the corresponding real parts),
// which for real inputs equals the full-spectrum definition exactly (the corner (N/2, N/2) lies outside the last ring).
#include "dg_internal.h"

namespace {

constexpr int RAPSD_PTS = 2048;                                     // complex points per workgroup and LDS buffer
constexpr int RAPSD_KQ = (DG_RAPSD_MAX_N / 2 + 1 + 255) / 256;      // rings per thread in the column pass

__host__ __device__ inline int isqrt_floor(int x) {
  int s = (int)sqrtf((float)x);
  while (s * s > x) --s;
  while ((s + 1) * (s + 1) <= x) ++s;
  return s;
}

// |v| range of ring k on line u: v^2 in [lo, hi] with r^2 = u^2 + v^2 in ring k.  Empty when vmin > vmax.
__host__ __device__ inline void ring_span(int u, int k, int N, int& vmin, int& vmax) {
  const int hi = k * k + k - u * u;
  if (hi < 0) { vmin = 1; vmax = 0; return; }
  int lo = (k == 0 ? 0 : k * k - k + 1) - u * u;
  lo = lo < 0 ? 0 : lo;
  vmax = isqrt_floor(hi);
  vmax = vmax > N / 2 ? N / 2 : vmax;
  vmin = isqrt_floor(lo);
  if (vmin * vmin < lo) ++vmin;
}

__host__ __device__ inline long long ring_count(int k, int N) {
  long long n = 0;
  for (int u = 0; u <= N / 2; ++u) {
    int vmin, vmax;
    ring_span(u, k, N, vmin, vmax);
    if (vmin > vmax) continue;
    long long nv = 2LL * (vmax - vmin + 1) - (vmin == 0) - (vmax == N / 2);   // v = 0 and v = -N/2 exist once
    n += (u == 0 || u == N / 2 ? 1 : 2) * nv;
  }
  return n;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// RAPSD_PTS / N forward complex FFTs of length N at once, Stockham autosort between buf[0] (input) and buf[1]; returns the
// buffer that holds the result (natural order).  Stage with span p and radix R: task i of an FFT (T = N / R tasks) reads
// x[i + j T], twiddles them by W^(j k N / (R p)) with k = i mod p, and writes the R-point DFT to y[(i - k) R + k + r p].
__device__ int fft_lds(float2 (*buf)[RAPSD_PTS], const float2* tw, int N, int logN) {
  const int nfft = RAPSD_PTS >> logN;
  int src = 0;
  for (int p = 1, logp = 0; p < N;) {
    const int R = (p * 4 <= N) ? 4 : 2, logR = R == 4 ? 2 : 1;
    const int logT = logN - logR, T = 1 << logT;
    const int tws = N >> (logp + logR);
    const float2* x = buf[src];
    float2* y = buf[src ^ 1];
    for (int task = threadIdx.x; task < nfft * T; task += 256) {
      const int j = task >> logT, i = task & (T - 1);
      const float2* xj = x + (j << logN);
      float2* yj = y + (j << logN);
      const int k = i & (p - 1), o = ((i - k) << logR) + k;
      if (R == 4) {
        const float2 u0 = xj[i];
        const float2 u1 = cmul(xj[i + T], tw[k * tws]);
        const float2 u2 = cmul(xj[i + 2 * T], tw[2 * k * tws]);
        const float2 u3 = cmul(xj[i + 3 * T], tw[3 * k * tws]);
        const float2 v0 = cadd(u0, u2), v1 = csub(u0, u2), v2 = cadd(u1, u3), d = csub(u1, u3);
        const float2 v3 = make_float2(d.y, -d.x);                   // -i (u1 - u3)
        yj[o] = cadd(v0, v2);
        yj[o + p] = cadd(v1, v3);
        yj[o + 2 * p] = csub(v0, v2);
        yj[o + 3 * p] = csub(v1, v3);
      } else {
        const float2 u0 = xj[i], u1 = cmul(xj[i + T], tw[k * tws]);
        yj[o] = cadd(u0, u1);
        yj[o + p] = csub(u0, u1);
      }
    }
    __syncthreads();
    src ^= 1;
    p <<= logR;
    logp += logR;
  }
  return src;
}

__global__ void rapsd_twiddle_kernel(float2* tw, int N) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= N) return;
  double s, c;
  sincospi(2.0 * m / N, &s, &c);
  tw[m] = make_float2((float)c, (float)-s);
}

__global__ void rapsd_count_kernel(double* cnt, int N) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k <= N / 2) cnt[k] = (double)ring_count(k, N);
}

struct RapsdRow {
  const void* base;
  long long ld_t, ld_c, ld_p;
  int C, N, logN;
  long long npairs;           // T * C * N / 2 row pairs
  const float2* tw;
  float2* spec;               // [F][N/2 + 1][N]
};

template <typename T>
__global__ __launch_bounds__(256) void rapsd_row_kernel(RapsdRow a) {
  __shared__ float2 buf[2][RAPSD_PTS];
  __shared__ float2 tw[DG_RAPSD_MAX_N];
  const int N = a.N, logN = a.logN, nfft = RAPSD_PTS >> logN, K = N / 2 + 1, half = N / 2;
  const long long g0 = (long long)blockIdx.x * nfft;
  for (int m = threadIdx.x; m < N; m += 256) tw[m] = a.tw[m];
  const T* base = reinterpret_cast<const T*>(a.base);
  for (int idx = threadIdx.x; idx < RAPSD_PTS; idx += 256) {
    const int j = idx >> logN, w = idx & (N - 1);
    const long long g = g0 + j;
    float2 z = make_float2(0.f, 0.f);
    if (g < a.npairs) {
      const long long f = g / half;
      const int h = 2 * (int)(g % half);
      const T* q = base + (f / a.C) * a.ld_t + (f % a.C) * a.ld_c + ((long long)h * N + w) * a.ld_p;
      z = make_float2(ld_elem(q), ld_elem(q + (long long)N * a.ld_p));
    }
    buf[0][idx] = z;
  }
  __syncthreads();
  const float2* Z = buf[fft_lds(buf, tw, N, logN)];
  // Z = A + i B for the rows (h, h + 1): A[u] = (Z[u] + conj Z[-u]) / 2, B[u] = -i (Z[u] - conj Z[-u]) / 2.  The pair index
  // runs fastest, so consecutive lanes store the adjacent rows h of one line u: spec[f][u][h .. h + 1] is one 16-byte store.
  for (int idx = threadIdx.x; idx < K * nfft; idx += 256) {
    const int u = idx >> (11 - logN), j = idx & (nfft - 1);
    const long long g = g0 + j;
    if (g >= a.npairs) continue;
    const float2 zu = Z[(j << logN) + u], zm = Z[(j << logN) + ((N - u) & (N - 1))];
    const float2 s = make_float2(0.5f * (zu.x + zm.x), 0.5f * (zu.y - zm.y));     // (Z[u] + conj Z[-u]) / 2
    const float2 d = make_float2(0.5f * (zu.x - zm.x), 0.5f * (zu.y + zm.y));     // (Z[u] - conj Z[-u]) / 2
    const long long f = g / half;
    const int h = 2 * (int)(g % half);
    *reinterpret_cast<float4*>(a.spec + (f * K + u) * N + h) = make_float4(s.x, s.y, d.y, -d.x);
  }
}

struct RapsdCol {
  const float2* spec;
  const float2* tw;
  int N, logN, S, L;          // S slices of L lines (a multiple of the FFTs per workgroup) per field
  double* part;               // [F][S][N/2 + 1]
};

__global__ __launch_bounds__(256) void rapsd_col_kernel(RapsdCol a) {
  __shared__ float2 buf[2][RAPSD_PTS];
  __shared__ float2 tw[DG_RAPSD_MAX_N];
  const int N = a.N, logN = a.logN, nfft = RAPSD_PTS >> logN, K = N / 2 + 1;
  const long long f = blockIdx.x / a.S;
  const int s = blockIdx.x % a.S;
  const int u_end = min(K, (s + 1) * a.L);
  const float inv = 1.f / ((float)N * (float)N);              // a power of two: exact
  for (int m = threadIdx.x; m < N; m += 256) tw[m] = a.tw[m];
  double acc[RAPSD_KQ];
#pragma unroll
  for (int q = 0; q < RAPSD_KQ; ++q) acc[q] = 0.0;
  for (int u0 = s * a.L; u0 < u_end; u0 += nfft) {
    const int nl = min(nfft, u_end - u0);
    const float4* src4 = reinterpret_cast<const float4*>(a.spec + (f * K + u0) * N);   // nl whole lines, contiguous
    for (int idx = threadIdx.x; idx < RAPSD_PTS / 2; idx += 256) {
      const float4 v = (2 * idx >> logN) < nl ? src4[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
      buf[0][2 * idx] = make_float2(v.x, v.y);
      buf[0][2 * idx + 1] = make_float2(v.z, v.w);
    }
    __syncthreads();
    const int r = fft_lds(buf, tw, N, logN);
    float* pw = reinterpret_cast<float*>(buf[r ^ 1]);
    for (int idx = threadIdx.x; idx < RAPSD_PTS; idx += 256) {
      const int u = u0 + (idx >> logN);
      const float2 X = buf[r][idx];
      pw[idx] = fmaf(X.x, X.x, X.y * X.y) * inv * (u == 0 || u == N / 2 ? 1.f : 2.f);
    }
    __syncthreads();
    for (int j = 0; j < nl; ++j) {
      const float* pl = pw + (j << logN);
#pragma unroll
      for (int q = 0; q < RAPSD_KQ; ++q) {
        const int k = threadIdx.x + 256 * q;
        if (k >= K) continue;
        int vmin, vmax;
        ring_span(u0 + j, k, N, vmin, vmax);
        double sum = 0.0;
        for (int v = vmin; v <= vmax; ++v) {
          sum += (double)pl[v];
          if (v != 0 && v != N / 2) sum += (double)pl[N - v];
        }
        acc[q] += sum;
      }
    }
    __syncthreads();                                            // the next batch overwrites buf
  }
  double* out = a.part + (f * a.S + s) * K;
#pragma unroll
  for (int q = 0; q < RAPSD_KQ; ++q) {
    const int k = threadIdx.x + 256 * q;
    if (k < K) out[k] = acc[q];
  }
}

// one thread per (field, ring): the slices in order
__global__ __launch_bounds__(256) void rapsd_field_kernel(const double* part, const double* cnt, long long F, int S, int K,
                                                          double* pf, double* per_field) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= F * K) return;
  const long long f = idx / K;
  const int k = (int)(idx % K);
  const double* q = part + f * S * K + k;
  double s = 0.0;
  for (int i = 0; i < S; ++i) s += q[(long long)i * K];
  s /= cnt[k];
  pf[idx] = s;
  if (per_field) per_field[idx] = s;
}

// one thread per (channel, ring): the fields in t order
__global__ __launch_bounds__(256) void rapsd_sum_kernel(const double* pf, int Tn, int C, int K, double* sum) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * K) return;
  double s = 0.0;
  for (int t = 0; t < Tn; ++t) s += pf[(long long)t * C * K + idx];
  sum[idx] = s;
}

struct CrossCol {
  const float2* spec_a;
  const float2* spec_b;
  const float2* tw;
  int N, logN, S, L;          // the slices of rapsd_ws
  double* part;               // [F][S][3][N/2 + 1]
};

// nl whole lines of one half spectrum (contiguous) into an LDS buffer, the rest of the buffer zero
__device__ __forceinline__ void cross_load_lines(float2* dst, const float2* lines, int nl, int logN) {
  const float4* src4 = reinterpret_cast<const float4*>(lines);
  for (int idx = threadIdx.x; idx < RAPSD_PTS / 2; idx += 256) {
    const float4 v = (2 * idx >> logN) < nl ? src4[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    dst[2 * idx] = make_float2(v.x, v.y);
    dst[2 * idx + 1] = make_float2(v.z, v.w);
  }
}

// LDS: buf[0], buf[1] are fft_lds's pair, buf[2] keeps side a's transformed lines while side b's run through the pair; after
// the products, planes 0 and 1 lie in the pair's free buffer and plane 2 over buf[2].  3 x 16 KB + 16 KB twiddles = 64 KB.
__global__ __launch_bounds__(256) void cross_col_kernel(CrossCol a) {
  __shared__ float2 buf[3][RAPSD_PTS];
  __shared__ float2 tw[DG_RAPSD_MAX_N];
  constexpr int PT = RAPSD_PTS / 256;                           // points per thread
  const int N = a.N, logN = a.logN, nfft = RAPSD_PTS >> logN, K = N / 2 + 1;
  const long long f = blockIdx.x / a.S;
  const int s = blockIdx.x % a.S;
  const int u_end = min(K, (s + 1) * a.L);
  const float inv = 1.f / ((float)N * (float)N);              // a power of two: exact
  for (int m = threadIdx.x; m < N; m += 256) tw[m] = a.tw[m];
  double acc[3][RAPSD_KQ];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < RAPSD_KQ; ++q) acc[p][q] = 0.0;
  for (int u0 = s * a.L; u0 < u_end; u0 += nfft) {
    const int nl = min(nfft, u_end - u0);
    const long long line0 = (f * K + u0) * N;
    cross_load_lines(buf[0], a.spec_a + line0, nl, logN);
    __syncthreads();
    int r = fft_lds(buf, tw, N, logN);
    for (int idx = threadIdx.x; idx < RAPSD_PTS; idx += 256) buf[2][idx] = buf[r][idx];
    __syncthreads();                                            // side b's lines overwrite buf[0]
    cross_load_lines(buf[0], a.spec_b + line0, nl, logN);
    __syncthreads();
    r = fft_lds(buf, tw, N, logN);
    float* pw = reinterpret_cast<float*>(buf[r ^ 1]);           // planes 0 and 1
    float co[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int u = u0 + (idx >> logN);
      const float w = u == 0 || u == N / 2 ? 1.f : 2.f;
      const float2 A = buf[2][idx], B = buf[r][idx];
      pw[idx] = fmaf(A.x, A.x, A.y * A.y) * inv * w;
      pw[RAPSD_PTS + idx] = fmaf(B.x, B.x, B.y * B.y) * inv * w;
      co[i] = fmaf(A.x, B.x, A.y * B.y) * inv * w;
    }
    __syncthreads();                                            // every A is read: plane 2 goes over buf[2]
    float* pc = reinterpret_cast<float*>(buf[2]);
#pragma unroll
    for (int i = 0; i < PT; ++i) pc[threadIdx.x + 256 * i] = co[i];
    __syncthreads();
    for (int j = 0; j < nl; ++j) {
      const float* pa = pw + (j << logN);
      const float* pb = pa + RAPSD_PTS;
      const float* pl = pc + (j << logN);
#pragma unroll
      for (int q = 0; q < RAPSD_KQ; ++q) {
        const int k = threadIdx.x + 256 * q;
        if (k >= K) continue;
        int vmin, vmax;
        ring_span(u0 + j, k, N, vmin, vmax);
        double sa = 0.0, sb = 0.0, sc = 0.0;
        for (int v = vmin; v <= vmax; ++v) {
          sa += (double)pa[v];
          sb += (double)pb[v];
          sc += (double)pl[v];
          if (v != 0 && v != N / 2) {
            sa += (double)pa[N - v];
            sb += (double)pb[N - v];
            sc += (double)pl[N - v];
          }
        }
        acc[0][q] += sa;
        acc[1][q] += sb;
        acc[2][q] += sc;
      }
    }
    __syncthreads();                                            // the next batch overwrites buf
  }
  double* out = a.part + (f * a.S + s) * 3 * K;
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < RAPSD_KQ; ++q) {
      const int k = threadIdx.x + 256 * q;
      if (k < K) out[p * K + k] = acc[p][q];
    }
}

// one thread per (field, plane, ring): the slices in order
__global__ __launch_bounds__(256) void cross_field_kernel(const double* part, const double* cnt, long long F, int S, int K,
                                                          double* pf, double* per_field) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= F * 3 * K) return;
  const long long f = idx / (3 * K);
  const int pk = (int)(idx % (3 * K));                          // plane * K + ring
  const double* q = part + f * S * 3 * K + pk;
  double s = 0.0;
  for (int i = 0; i < S; ++i) s += q[(long long)i * 3 * K];
  s /= cnt[pk % K];
  pf[idx] = s;
  if (per_field) per_field[idx] = s;
}

// one thread per (channel, plane, ring): the fields in t order
__global__ __launch_bounds__(256) void cross_sum_kernel(const double* pf, int Tn, int C, int K, double* sum) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * 3 * K) return;
  double s = 0.0;
  for (int t = 0; t < Tn; ++t) s += pf[(long long)t * C * 3 * K + idx];
  sum[idx] = s;
}

struct HelmCol {
  const float2* spec[4];      // half spectra of (u, v) of side a, then of side b (one-sided: the first two)
  const float2* tw;
  float su, sv;               // per-component scale
  int N, logN, S, L;          // the slices of rapsd_ws
  double* part;               // [F][S][NP][N/2 + 1], NP = 3 or 8
};

constexpr int HELM_PT = RAPSD_PTS / 256;                        // points per thread and batch

// What a point idx of a batch that starts at line u0 needs: the signed wavenumbers (kx = u along W, ky along H), whether the
// Nyquist rule applies, gk = weight / (2 N^2) and g = gk / k2 (0 at k2 = 0: the mean has neither part).
struct HelmGeom {
  float kx, ky, gk, g;
  bool nyq;
};

__device__ __forceinline__ HelmGeom helm_geom(int idx, int u0, int N, int logN) {
  const int u = u0 + (idx >> logN), v = idx & (N - 1);
  const int sv = v <= N / 2 ? v : v - N;
  const int k2 = u * u + sv * sv;
  HelmGeom h;
  h.kx = (float)u;
  h.ky = (float)sv;
  h.nyq = u == N / 2 || v == N / 2;
  h.gk = 0.5f / ((float)N * (float)N) * (u == 0 || u == N / 2 ? 1.f : 2.f);   // powers of two: exact
  h.g = k2 > 0 ? h.gk / (float)k2 : 0.f;
  return h;
}

// The rotational and divergent co-products of one point, R = kx V - ky U, D = kx U + ky V of each side:
//   rot = Re(Ra conj Rb) g,  div = Re(Da conj Db) g;  on a Nyquist line (see the header) the sum without the cross term:
//   rot = (kx^2 Re(Va conj Vb) + ky^2 Re(Ua conj Ub)) g,  div = (kx^2 Re(Ua conj Ub) + ky^2 Re(Va conj Vb)) g.
// Called with b = a it gives a side's own rot and div, by the same operations: the co-planes of (a, a) equal a's planes.
__device__ __forceinline__ void helm_products(const HelmGeom& h, float2 Ua, float2 Va, float2 Ub, float2 Vb, float& rot,
                                              float& div) {
  if (h.nyq) {
    const float uu = fmaf(Ua.x, Ub.x, Ua.y * Ub.y), vv = fmaf(Va.x, Vb.x, Va.y * Vb.y);
    const float kx2 = h.kx * h.kx, ky2 = h.ky * h.ky;
    rot = fmaf(kx2, vv, ky2 * uu) * h.g;
    div = fmaf(kx2, uu, ky2 * vv) * h.g;
  } else {
    const float2 Ra = make_float2(fmaf(h.kx, Va.x, -(h.ky * Ua.x)), fmaf(h.kx, Va.y, -(h.ky * Ua.y)));
    const float2 Rb = make_float2(fmaf(h.kx, Vb.x, -(h.ky * Ub.x)), fmaf(h.kx, Vb.y, -(h.ky * Ub.y)));
    const float2 Da = make_float2(fmaf(h.kx, Ua.x, h.ky * Va.x), fmaf(h.kx, Ua.y, h.ky * Va.y));
    const float2 Db = make_float2(fmaf(h.kx, Ub.x, h.ky * Vb.x), fmaf(h.kx, Ub.y, h.ky * Vb.y));
    rot = fmaf(Ra.x, Rb.x, Ra.y * Rb.y) * h.g;
    div = fmaf(Da.x, Db.x, Da.y * Db.y) * h.g;
  }
}

// One side of a batch: nl lines of U^ and of V^ through fft_lds (U^'s transformed lines parked in buf[2] as in
// cross_col_kernel), then each thread's HELM_PT points (idx = threadIdx.x + 256 i, the same points in every batch and for
// either side): the scaled U, V and their ke, rot, div in fp32.  ke and rot go straight into the FFT's free buffer, div waits
// in registers until every thread has read its U and V and then goes over buf[2].  MODE 0: nothing else.  MODE 1 (side a of a
// pair): the scaled U, V are handed out in Ua, Va.  MODE 2 (side b): the co-products with the Ua, Va handed in are formed next
// to b's own and stored as planes 3 and 4.  Ends behind a barrier with pl[] = the planes (RAPSD_PTS floats each).
template <int MODE>
__device__ __forceinline__ void helm_side(float2 (*buf)[RAPSD_PTS], const float2* tw, const float2* lu, const float2* lv, int nl,
                                          int u0, int N, int logN, float su, float sv, float2 (&Ua)[HELM_PT], float2 (&Va)[HELM_PT],
                                          const float* (&pl)[5]) {
  cross_load_lines(buf[0], lu, nl, logN);
  __syncthreads();
  int r = fft_lds(buf, tw, N, logN);
  for (int idx = threadIdx.x; idx < RAPSD_PTS; idx += 256) buf[2][idx] = buf[r][idx];
  __syncthreads();                                              // V^'s lines overwrite buf[0]
  cross_load_lines(buf[0], lv, nl, logN);
  __syncthreads();
  r = fft_lds(buf, tw, N, logN);
  float* free1 = reinterpret_cast<float*>(buf[r ^ 1]);          // the last stage's source: nobody reads it any more
  float div[HELM_PT], co_rot[HELM_PT], co_div[HELM_PT];
#pragma unroll
  for (int i = 0; i < HELM_PT; ++i) {
    const int idx = threadIdx.x + 256 * i;
    const float2 x = buf[2][idx], y = buf[r][idx];
    const float2 U = make_float2(x.x * su, x.y * su), V = make_float2(y.x * sv, y.y * sv);
    const HelmGeom h = helm_geom(idx, u0, N, logN);
    float rot;
    helm_products(h, U, V, U, V, rot, div[i]);
    free1[idx] = (fmaf(U.x, U.x, U.y * U.y) + fmaf(V.x, V.x, V.y * V.y)) * h.gk;
    free1[RAPSD_PTS + idx] = rot;
    if (MODE == 1) { Ua[i] = U; Va[i] = V; }
    if (MODE == 2) helm_products(h, Ua[i], Va[i], U, V, co_rot[i], co_div[i]);
  }
  __syncthreads();                                              // every U and V is read: planes go over buf[2] and buf[r]
  float* free2 = reinterpret_cast<float*>(buf[2]);
  float* free3 = reinterpret_cast<float*>(buf[r]);
#pragma unroll
  for (int i = 0; i < HELM_PT; ++i) {
    const int idx = threadIdx.x + 256 * i;
    free2[idx] = div[i];
    if (MODE == 2) {
      free2[RAPSD_PTS + idx] = co_rot[i];
      free3[idx] = co_div[i];
    }
  }
  __syncthreads();
  pl[0] = free1; pl[1] = free1 + RAPSD_PTS; pl[2] = free2; pl[3] = free2 + RAPSD_PTS; pl[4] = free3;
}

// Ring sums of planes pl[P0 .. P0 + NP) (LDS, RAPSD_PTS floats each) over the nl lines of a batch: rapsd_col_kernel's loop order
// and fp64 accumulation, one independent sum per plane, so a plane's bits do not depend on which planes are summed next to it.
template <int P0, int NP>
__device__ __forceinline__ void helm_ring_sums(const float* const (&pl)[5], int u0, int nl, int N, int logN, int K,
                                               double (*acc)[RAPSD_KQ]) {
  for (int j = 0; j < nl; ++j) {
    const int o = j << logN;
#pragma unroll
    for (int q = 0; q < RAPSD_KQ; ++q) {
      const int k = threadIdx.x + 256 * q;
      if (k >= K) continue;
      int vmin, vmax;
      ring_span(u0 + j, k, N, vmin, vmax);
      double s[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) s[p] = 0.0;
      for (int v = vmin; v <= vmax; ++v) {
#pragma unroll
        for (int p = 0; p < NP; ++p) s[p] += (double)pl[P0 + p][o + v];
        if (v != 0 && v != N / 2) {
#pragma unroll
          for (int p = 0; p < NP; ++p) s[p] += (double)pl[P0 + p][o + N - v];
        }
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p][q] += s[p];
    }
  }
}

template <int NP>
__device__ __forceinline__ void helm_write_part(double* out, int K, const double (*acc)[RAPSD_KQ]) {
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int q = 0; q < RAPSD_KQ; ++q) {
      const int k = threadIdx.x + 256 * q;
      if (k < K) out[p * K + k] = acc[p][q];
    }
}

// One-sided Helmholtz spectra.  LDS as cross_col_kernel: 3 x 16 KB line buffers + 16 KB twiddles = 64 KB, two workgroups per CU.
__global__ __launch_bounds__(256, 2) void helm_col_kernel(HelmCol a) {
  __shared__ float2 buf[3][RAPSD_PTS];
  __shared__ float2 tw[DG_RAPSD_MAX_N];
  const int N = a.N, logN = a.logN, nfft = RAPSD_PTS >> logN, K = N / 2 + 1;
  const long long f = blockIdx.x / a.S;
  const int s = blockIdx.x % a.S;
  const int u_end = min(K, (s + 1) * a.L);
  for (int m = threadIdx.x; m < N; m += 256) tw[m] = a.tw[m];
  double acc[3][RAPSD_KQ];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < RAPSD_KQ; ++q) acc[p][q] = 0.0;
  for (int u0 = s * a.L; u0 < u_end; u0 += nfft) {
    const int nl = min(nfft, u_end - u0);
    const long long line0 = (f * K + u0) * N;
    float2 U[HELM_PT], V[HELM_PT];                              // unused in MODE 0
    const float* pl[5];
    helm_side<0>(buf, tw, a.spec[0] + line0, a.spec[1] + line0, nl, u0, N, logN, a.su, a.sv, U, V, pl);
    helm_ring_sums<0, 3>(pl, u0, nl, N, logN, K, acc);
    __syncthreads();                                            // the next batch overwrites buf
  }
  helm_write_part<3>(a.part + (f * a.S + s) * 3 * K, K, acc);
}

// Paired Helmholtz spectra, planes [ke_a, rot_a, div_a, ke_b, rot_b, div_b, co_rot, co_div].  Side a runs first and is ring-summed
// exactly as in helm_col_kernel; its scaled U, V stay in registers (4 floats x HELM_PT points = 32 VGPRs: R and D follow from
// them, and the Nyquist rule needs the components themselves) while side b runs through the same three LDS buffers.  Side b's
// three planes and the two co-planes are then ring-summed in one walk over the lines.  LDS stays at 64 KB; the accumulators are
// 8 x RAPSD_KQ doubles per thread, all eight planes in one pass: 248 VGPRs, no spill at two workgroups per CU.
__global__ __launch_bounds__(256, 2) void helm_cross_col_kernel(HelmCol a) {
  __shared__ float2 buf[3][RAPSD_PTS];
  __shared__ float2 tw[DG_RAPSD_MAX_N];
  const int N = a.N, logN = a.logN, nfft = RAPSD_PTS >> logN, K = N / 2 + 1;
  const long long f = blockIdx.x / a.S;
  const int s = blockIdx.x % a.S;
  const int u_end = min(K, (s + 1) * a.L);
  for (int m = threadIdx.x; m < N; m += 256) tw[m] = a.tw[m];
  double acc[8][RAPSD_KQ];
#pragma unroll
  for (int p = 0; p < 8; ++p)
#pragma unroll
    for (int q = 0; q < RAPSD_KQ; ++q) acc[p][q] = 0.0;
  for (int u0 = s * a.L; u0 < u_end; u0 += nfft) {
    const int nl = min(nfft, u_end - u0);
    const long long line0 = (f * K + u0) * N;
    float2 Ua[HELM_PT], Va[HELM_PT];
    const float* pl[5];
    helm_side<1>(buf, tw, a.spec[0] + line0, a.spec[1] + line0, nl, u0, N, logN, a.su, a.sv, Ua, Va, pl);
    helm_ring_sums<0, 3>(pl, u0, nl, N, logN, K, acc);
    __syncthreads();                                            // side b's lines overwrite buf
    helm_side<2>(buf, tw, a.spec[2] + line0, a.spec[3] + line0, nl, u0, N, logN, a.su, a.sv, Ua, Va, pl);
    helm_ring_sums<0, 5>(pl, u0, nl, N, logN, K, acc + 3);
    __syncthreads();                                            // the next batch overwrites buf
  }
  helm_write_part<8>(a.part + (f * a.S + s) * 8 * K, K, acc);
}

// one thread per (field, plane, ring): the slices in order (cross_field_kernel for NP planes)
__global__ __launch_bounds__(256) void helm_field_kernel(const double* part, const double* cnt, long long F, int S, int NP, int K,
                                                         double* pf, double* per_field) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= F * NP * K) return;
  const long long f = idx / (NP * K);
  const int pk = (int)(idx % (NP * K));                         // plane * K + ring
  const double* q = part + f * S * NP * K + pk;
  double s = 0.0;
  for (int i = 0; i < S; ++i) s += q[(long long)i * NP * K];
  s /= cnt[pk % K];
  pf[idx] = s;
  if (per_field) per_field[idx] = s;
}

// one thread per (plane, ring): the fields in t order
__global__ __launch_bounds__(256) void helm_sum_kernel(const double* pf, int Tn, int NPK, double* sum) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= NPK) return;
  double s = 0.0;
  for (int t = 0; t < Tn; ++t) s += pf[(long long)t * NPK + idx];
  sum[idx] = s;
}

// workspace: twiddles, counts, spec, slice partials, per-field spectra (each 256-byte aligned)
struct RapsdWs {
  size_t tw, cnt, spec, part, pf, bytes;
  int S, L;
};

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool rapsd_n_ok(int N) { return N >= 16 && N <= DG_RAPSD_MAX_N && (N & (N - 1)) == 0; }

RapsdWs rapsd_ws(long long F, int N) {
  RapsdWs w;
  const int K = N / 2 + 1, nfft = RAPSD_PTS / N;
  const int nb = (K + nfft - 1) / nfft;                         // line batches per field
  long long S = (2048 + F - 1) / F;                             // ~2048 column workgroups
  S = S < 1 ? 1 : S > nb ? nb : S;
  w.S = (int)S;
  w.L = (nb + w.S - 1) / w.S * nfft;
  w.tw = 0;
  w.cnt = w.tw + align256((size_t)N * 8);
  w.spec = w.cnt + align256((size_t)K * 8);
  w.part = w.spec + align256((size_t)F * K * N * 8);
  w.pf = w.part + align256((size_t)F * w.S * K * 8);
  w.bytes = w.pf + align256((size_t)F * K * 8);
  return w;
}

// cross spectra: twiddles, counts, both sides' spec, slice partials [F][S][3][K], per-field [F][3][K]; S and L as rapsd_ws
struct CrossWs {
  size_t tw, cnt, spec_a, spec_b, part, pf, bytes;
  int S, L;
};

CrossWs cross_ws(long long F, int N) {
  const RapsdWs r = rapsd_ws(F, N);
  const int K = N / 2 + 1;
  CrossWs w;
  w.S = r.S;
  w.L = r.L;
  w.tw = 0;
  w.cnt = w.tw + align256((size_t)N * 8);
  w.spec_a = w.cnt + align256((size_t)K * 8);
  w.spec_b = w.spec_a + align256((size_t)F * K * N * 8);
  w.part = w.spec_b + align256((size_t)F * K * N * 8);
  w.pf = w.part + align256((size_t)F * w.S * 3 * K * 8);
  w.bytes = w.pf + align256((size_t)F * 3 * K * 8);
  return w;
}

bool rapsd_fields_ok(const dg_eof_fields* x, int N) {
  return x && x->base && x->T >= 1 && x->C >= 1 && x->C <= DG_EOF_MAX_C && x->P == N * N && x->ld_t >= 0 && x->ld_c >= 0 &&
         x->ld_p >= 0;
}

void launch_row(const dg_eof_fields* x, int N, long long npairs, long long row_blocks, const float2* tw, float2* spec,
                hipStream_t st) {
  RapsdRow r;
  r.base = x->base; r.ld_t = x->ld_t; r.ld_c = x->ld_c; r.ld_p = x->ld_p;
  r.C = x->C; r.N = N; r.logN = __builtin_ctz(N); r.npairs = npairs; r.tw = tw; r.spec = spec;
  if (x->dtype == DG_F32) hipLaunchKernelGGL(rapsd_row_kernel<float>, dim3((unsigned)row_blocks), dim3(256), 0, st, r);
  else hipLaunchKernelGGL(rapsd_row_kernel<bf16_t>, dim3((unsigned)row_blocks), dim3(256), 0, st, r);
}

// Helmholtz spectra: twiddles, counts, the half spectra of (u, v) of each side, slice partials [T][S][NP][K], per-field
// [T][NP][K]; one field per pair, so S and L are rapsd_ws(T, N)'s
struct HelmWs {
  size_t tw, cnt, spec[4], part, pf, bytes;
  int S, L;
};

HelmWs helm_ws(long long T, int N, int sides) {
  const RapsdWs r = rapsd_ws(T, N);
  const int K = N / 2 + 1, NP = sides == 2 ? 8 : 3;
  HelmWs w;
  w.S = r.S;
  w.L = r.L;
  w.tw = 0;
  w.cnt = w.tw + align256((size_t)N * 8);
  size_t at = w.cnt + align256((size_t)K * 8);
  for (int i = 0; i < 4; ++i) {
    w.spec[i] = at;
    if (i < 2 * sides) at += align256((size_t)T * K * N * 8);
  }
  w.part = at;
  w.pf = w.part + align256((size_t)T * w.S * NP * K * 8);
  w.bytes = w.pf + align256((size_t)T * NP * K * 8);
  return w;
}

bool helm_side_ok(const dg_eof_fields* x, int cu, int cv, int N) {
  return rapsd_fields_ok(x, N) && cu >= 0 && cv >= 0 && cu != cv && cu < x->C && cv < x->C;
}

// the one-channel descriptor of channel c of x
dg_eof_fields helm_channel(const dg_eof_fields* x, int c) {
  dg_eof_fields y = *x;
  y.base = reinterpret_cast<const char*>(x->base) + (long long)c * x->ld_c * (x->dtype == DG_F32 ? 4 : 2);
  y.C = 1;
  return y;
}

int helm_run(const dg_eof_fields* a, const dg_eof_fields* b, int cu, int cv, const float* scale, int N, void* ws,
             double* per_field, double* sum, void* stream) {
  const int sides = b ? 2 : 1, NP = b ? 8 : 3;
  const long long T = a->T;
  const int K = N / 2 + 1, logN = __builtin_ctz(N), nfft = RAPSD_PTS / N;
  const HelmWs w = helm_ws(T, N, sides);
  const long long npairs = T * (N / 2);
  const long long row_blocks = (npairs + nfft - 1) / nfft, col_blocks = T * w.S;
  if (row_blocks > 0x7fffffffLL || col_blocks > 0x7fffffffLL || T * NP * K > 0x7fffffffLL * 256LL) return DG_ERR_BAD_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = reinterpret_cast<char*>(ws);
  float2* tw = reinterpret_cast<float2*>(base + w.tw);
  double* cnt = reinterpret_cast<double*>(base + w.cnt);
  double* part = reinterpret_cast<double*>(base + w.part);
  double* pf = reinterpret_cast<double*>(base + w.pf);
  hipLaunchKernelGGL(rapsd_twiddle_kernel, dim3((N + 255) / 256), dim3(256), 0, st, tw, N);
  hipLaunchKernelGGL(rapsd_count_kernel, dim3((K + 255) / 256), dim3(256), 0, st, cnt, N);
  HelmCol c;
  for (int i = 0; i < 4; ++i) c.spec[i] = reinterpret_cast<float2*>(base + w.spec[i]);
  for (int i = 0; i < 2 * sides; ++i) {
    const dg_eof_fields x = helm_channel(i < 2 ? a : b, i % 2 ? cv : cu);
    launch_row(&x, N, npairs, row_blocks, tw, reinterpret_cast<float2*>(base + w.spec[i]), st);
  }
  c.tw = tw; c.su = scale[0]; c.sv = scale[1]; c.N = N; c.logN = logN; c.S = w.S; c.L = w.L; c.part = part;
  if (b) hipLaunchKernelGGL(helm_cross_col_kernel, dim3((unsigned)col_blocks), dim3(256), 0, st, c);
  else hipLaunchKernelGGL(helm_col_kernel, dim3((unsigned)col_blocks), dim3(256), 0, st, c);
  hipLaunchKernelGGL(helm_field_kernel, dim3((unsigned)((T * NP * K + 255) / 256)), dim3(256), 0, st, (const double*)part,
                     (const double*)cnt, T, w.S, NP, K, pf, per_field);
  if (sum)
    hipLaunchKernelGGL(helm_sum_kernel, dim3((unsigned)((NP * K + 255) / 256)), dim3(256), 0, st, (const double*)pf, (int)T, NP * K,
                       sum);
  return dg_check_launch();
}

bool helm_scale_ok(const float* scale) {
  return scale && std::isfinite(scale[0]) && std::isfinite(scale[1]) && scale[0] != 0.f && scale[1] != 0.f;
}

}  // namespace

extern "C" size_t dg_helmholtz_ws_bytes(int T, int N) {
  if (T < 1 || !rapsd_n_ok(N)) return 0;
  return helm_ws(T, N, 1).bytes;
}

extern "C" int dg_helmholtz(const dg_eof_fields* x, int cu, int cv, const float scale[2], int N, void* ws, double* per_field,
                            double* sum, void* stream) {
  if (!ws || !rapsd_n_ok(N) || !helm_side_ok(x, cu, cv, N) || !helm_scale_ok(scale)) return DG_ERR_BAD_SHAPE;
  if (x->dtype != DG_F32 && x->dtype != DG_BF16) return DG_ERR_BAD_DTYPE;
  return helm_run(x, nullptr, cu, cv, scale, N, ws, per_field, sum, stream);
}

extern "C" size_t dg_helmholtz_cross_ws_bytes(int T, int N) {
  if (T < 1 || !rapsd_n_ok(N)) return 0;
  return helm_ws(T, N, 2).bytes;
}

extern "C" int dg_helmholtz_cross(const dg_eof_fields* a, const dg_eof_fields* b, int cu, int cv, const float scale[2], int N,
                                  void* ws, double* per_field, double* sum, void* stream) {
  if (!ws || !rapsd_n_ok(N) || !helm_side_ok(a, cu, cv, N) || !helm_side_ok(b, cu, cv, N) || a->T != b->T || a->C != b->C ||
      !helm_scale_ok(scale))
    return DG_ERR_BAD_SHAPE;
  if ((a->dtype != DG_F32 && a->dtype != DG_BF16) || (b->dtype != DG_F32 && b->dtype != DG_BF16)) return DG_ERR_BAD_DTYPE;
  return helm_run(a, b, cu, cv, scale, N, ws, per_field, sum, stream);
}

extern "C" size_t dg_rapsd_ws_bytes(int T, int C, int N) {
  if (T < 1 || C < 1 || C > DG_EOF_MAX_C || !rapsd_n_ok(N)) return 0;
  return rapsd_ws((long long)T * C, N).bytes;
}

extern "C" int dg_rapsd_ring_counts(int N, int64_t* counts) {
  if (!rapsd_n_ok(N) || !counts) return DG_ERR_BAD_SHAPE;
  for (int k = 0; k <= N / 2; ++k) counts[k] = ring_count(k, N);
  return DG_OK;
}

extern "C" int dg_rapsd(const dg_eof_fields* x, int N, void* ws, double* per_field, double* sum, void* stream) {
  if (!ws || !rapsd_n_ok(N) || !rapsd_fields_ok(x, N)) return DG_ERR_BAD_SHAPE;
  if (x->dtype != DG_F32 && x->dtype != DG_BF16) return DG_ERR_BAD_DTYPE;
  const long long F = (long long)x->T * x->C;
  const int K = N / 2 + 1, logN = __builtin_ctz(N), nfft = RAPSD_PTS / N;
  const RapsdWs w = rapsd_ws(F, N);
  const long long npairs = F * (N / 2);
  const long long row_blocks = (npairs + nfft - 1) / nfft, col_blocks = F * w.S;
  if (row_blocks > 0x7fffffffLL || col_blocks > 0x7fffffffLL || F * K > 0x7fffffffLL * 256LL) return DG_ERR_BAD_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* b = reinterpret_cast<char*>(ws);
  float2* tw = reinterpret_cast<float2*>(b + w.tw);
  double* cnt = reinterpret_cast<double*>(b + w.cnt);
  float2* spec = reinterpret_cast<float2*>(b + w.spec);
  double* part = reinterpret_cast<double*>(b + w.part);
  double* pf = reinterpret_cast<double*>(b + w.pf);
  hipLaunchKernelGGL(rapsd_twiddle_kernel, dim3((N + 255) / 256), dim3(256), 0, st, tw, N);
  hipLaunchKernelGGL(rapsd_count_kernel, dim3((K + 255) / 256), dim3(256), 0, st, cnt, N);
  launch_row(x, N, npairs, row_blocks, tw, spec, st);
  RapsdCol c;
  c.spec = spec; c.tw = tw; c.N = N; c.logN = logN; c.S = w.S; c.L = w.L; c.part = part;
  hipLaunchKernelGGL(rapsd_col_kernel, dim3((unsigned)col_blocks), dim3(256), 0, st, c);
  hipLaunchKernelGGL(rapsd_field_kernel, dim3((unsigned)((F * K + 255) / 256)), dim3(256), 0, st, (const double*)part,
                     (const double*)cnt, F, w.S, K, pf, per_field);
  if (sum)
    hipLaunchKernelGGL(rapsd_sum_kernel, dim3((unsigned)((x->C * K + 255) / 256)), dim3(256), 0, st, (const double*)pf, x->T, x->C,
                       K, sum);
  return dg_check_launch();
}

extern "C" size_t dg_cross_rapsd_ws_bytes(int T, int C, int N) {
  if (T < 1 || C < 1 || C > DG_EOF_MAX_C || !rapsd_n_ok(N)) return 0;
  return cross_ws((long long)T * C, N).bytes;
}

extern "C" int dg_cross_rapsd(const dg_eof_fields* a, const dg_eof_fields* b, int N, void* ws, double* per_field, double* sum,
                              void* stream) {
  if (!ws || !rapsd_n_ok(N) || !rapsd_fields_ok(a, N) || !rapsd_fields_ok(b, N) || a->T != b->T || a->C != b->C)
    return DG_ERR_BAD_SHAPE;
  if ((a->dtype != DG_F32 && a->dtype != DG_BF16) || (b->dtype != DG_F32 && b->dtype != DG_BF16)) return DG_ERR_BAD_DTYPE;
  const long long F = (long long)a->T * a->C;
  const int K = N / 2 + 1, logN = __builtin_ctz(N), nfft = RAPSD_PTS / N;
  const CrossWs w = cross_ws(F, N);
  const long long npairs = F * (N / 2);
  const long long row_blocks = (npairs + nfft - 1) / nfft, col_blocks = F * w.S;
  if (row_blocks > 0x7fffffffLL || col_blocks > 0x7fffffffLL || F * 3 * K > 0x7fffffffLL * 256LL) return DG_ERR_BAD_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = reinterpret_cast<char*>(ws);
  float2* tw = reinterpret_cast<float2*>(base + w.tw);
  double* cnt = reinterpret_cast<double*>(base + w.cnt);
  float2* spec_a = reinterpret_cast<float2*>(base + w.spec_a);
  float2* spec_b = reinterpret_cast<float2*>(base + w.spec_b);
  double* part = reinterpret_cast<double*>(base + w.part);
  double* pf = reinterpret_cast<double*>(base + w.pf);
  hipLaunchKernelGGL(rapsd_twiddle_kernel, dim3((N + 255) / 256), dim3(256), 0, st, tw, N);
  hipLaunchKernelGGL(rapsd_count_kernel, dim3((K + 255) / 256), dim3(256), 0, st, cnt, N);
  launch_row(a, N, npairs, row_blocks, tw, spec_a, st);
  launch_row(b, N, npairs, row_blocks, tw, spec_b, st);
  CrossCol c;
  c.spec_a = spec_a; c.spec_b = spec_b; c.tw = tw; c.N = N; c.logN = logN; c.S = w.S; c.L = w.L; c.part = part;
  hipLaunchKernelGGL(cross_col_kernel, dim3((unsigned)col_blocks), dim3(256), 0, st, c);
  hipLaunchKernelGGL(cross_field_kernel, dim3((unsigned)((F * 3 * K + 255) / 256)), dim3(256), 0, st, (const double*)part,
                     (const double*)cnt, F, w.S, K, pf, per_field);
  if (sum)
    hipLaunchKernelGGL(cross_sum_kernel, dim3((unsigned)((a->C * 3 * K + 255) / 256)), dim3(256), 0, st, (const double*)pf, a->T,
                       a->C, K, sum);
  return dg_check_launch();
}
