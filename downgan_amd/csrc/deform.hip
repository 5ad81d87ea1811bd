// Field-deformation verification (include/downgan_hip.h "Field-deformation verification") of two series of H x W fields read through
// the EOF descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16): per output channel j and direction (0: target a, source b;
// 1: target b, source a) the displacement field d_0 of the pyramidal matcher of Keil & Craig, and from it the exact integer sums
// (the table of displacement vectors over the target's non-empty pixels, and five scalars) of the displacement / amplitude score.
//   deform_quant_kernel<T, MODE>   one launch per series: a thread takes one pixel, forms the output values y of hist_common.h and
//                                  writes q = the 8-bit code of every output channel into level 0 of the (t, j, side) pyramid
//   deform_down_kernel<SRC>        one launch per level l = 1 .. F: P_l = the sums of the 2 x 2 blocks of P_(l-1) (uint16)
//   deform_match_kernel<PIX, COST> one launch per level l = F .. 0, both directions of every (t, j): a workgroup of four waves owns
//                                  a 64 x 32 tile; X_l (halo 2), Y' (halo 4: one gather through the parent's displacement each)
//                                  and init (halo 2) are staged in LDS.  A thread owns one column of 8 pixels and keeps the 12 x 5
//                                  values of X_l around it in registers.  For each of the 25 shifts, in the tie order, it sums the
//                                  squared differences of the 5 pixels of each of its 12 rows once, slides the sum of 5 rows down
//                                  the column, and keeps the best (cost, shift) of each pixel with a strict <: the loop order is the
//                                  tie rule.  No barrier inside the shift loop.
//   deform_sums_kernel             a workgroup takes one (j, direction) and a slice of the pixels of all fields: M = Y_0[p + d_0],
//                                  the displacement table as an LDS histogram flushed by one 64-bit atomic per non-zero bin, the
//                                  five scalars by wave shuffles and one atomic each
//   deform_emit_kernel             dg_deform_field: d_0 as planar int16 and M as uint8
// No float after the quantiser and integer atomics only: exact, and two calls on the same data are bit-identical.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int DEF_TW = 64, DEF_TH = 32;               // the tile of a workgroup: a wave's lanes along x, 8 rows per wave
constexpr int DEF_THREADS = 256, DEF_STRIP = 8;       // a thread's column of pixels
static_assert(DEF_TW == 64 && DEF_TH == (DEF_THREADS / 64) * DEF_STRIP, "a lane per column, a strip per wave");
constexpr int DEF_R = 2;                              // shifts and window offsets are -2 .. 2
constexpr int DEF_XW = DEF_TW + 2 * DEF_R, DEF_XH = DEF_TH + 2 * DEF_R;          // X_l and init with a halo of 2
constexpr int DEF_YW = DEF_TW + 4 * DEF_R, DEF_YH = DEF_TH + 4 * DEF_R;          // Y' with a halo of 4
constexpr int DEF_ROWS = DEF_STRIP + 2 * DEF_R;       // rows of X_l a thread's strip touches
constexpr int DEF_GRID_Z = 32768;                     // planes / fields across gridDim.y at most; the kernels stride over the rest
constexpr int MAXO = DG_HIST_MAX_OUT, MAXL = DG_DEFORM_MAX_LEVELS;
constexpr int DEF_QBINS = 254;                        // inner bins of the quantiser: codes 1 .. 254
constexpr long long DEF_LIMIT = 1LL << 62, DEF_PIX_LIMIT = 1LL << 31;
constexpr long long DEF_FIELD_MAX = 255LL * 255LL;    // the most one pixel adds to any sum
// the LDS displacement table of deform_sums_kernel: (2 D + 1)^2 uint32, 62500 bytes at F = 4
static_assert((2 * (2 * ((2 << MAXL) - 1)) + 1) * (2 * (2 * ((2 << MAXL) - 1)) + 1) * 4 <= 64 * 1024, "the displacement table fits LDS");

typedef unsigned long long u64;
typedef unsigned short u16;
typedef unsigned char u8;

// the 25 shifts (sy, sx) sorted by (sy^2 + sx^2, sy, sx): the order of the matching loop, hence the tie rule
// (ints: the loop reads a row with one scalar load)
__constant__ int DEF_SHIFT[25][2] = {
    {0, 0},
    {-1, 0}, {0, -1}, {0, 1}, {1, 0},
    {-1, -1}, {-1, 1}, {1, -1}, {1, 1},
    {-2, 0}, {0, -2}, {0, 2}, {2, 0},
    {-2, -1}, {-2, 1}, {-1, -2}, {-1, 2}, {1, -2}, {1, 2}, {2, -1}, {2, 1},
    {-2, -2}, {-2, 2}, {2, -2}, {2, 2}};

__host__ __device__ inline unsigned def_pack(int dy, int dx) { return ((unsigned)dy & 0xffffu) | ((unsigned)dx << 16); }
__host__ __device__ inline int def_dy(unsigned v) { return (int)(short)(v & 0xffffu); }
__host__ __device__ inline int def_dx(unsigned v) { return (int)(short)(v >> 16); }

// the quantiser of the definition
__host__ __device__ inline unsigned def_quant(float y, float lo, float inv_step) {
  const int b = hist_bin(y, lo, inv_step, DEF_QBINS);
  return b > DEF_QBINS + 1 ? 0u : (unsigned)b;        // 0 underflow, 1 .. 254, 255 overflow; the NaN code 256 -> 0
}

struct DefQuantArgs {
  HistSeries x;
  HistXform xf;
  int P, T, nout, side;
  float lo[MAXO], inv_step[MAXO];
  u8* pyr;
  size_t plane;                                       // bytes of one (t, j, side) pyramid
};

template <typename T, int MODE>
__global__ __launch_bounds__(256) void deform_quant_kernel(DefQuantArgs g) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= g.P) return;
  const T* base = reinterpret_cast<const T*>(g.x.base);
  for (int t = blockIdx.y; t < g.T; t += gridDim.y) {
    float y[MAXO];
    hist_pixel_values<T, MODE>(g.xf, base + t * g.x.ld_t + p * g.x.ld_p, g.x.ld_c, y);
#pragma unroll
    for (int j = 0; j < MAXO; ++j)
      if (j < g.nout) g.pyr[(((size_t)t * g.nout + j) * 2 + g.side) * g.plane + p] = (u8)def_quant(y[j], g.lo[j], g.inv_step[j]);
  }
}

template <typename SRC>
__global__ __launch_bounds__(256) void deform_down_kernel(u8* pyr, size_t plane, size_t src_off, size_t dst_off, int hs, int ws, int hd,
                                                          int wd, long long planes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hd * wd) return;
  const int y = i / wd, x = i % wd;
  const bool right = 2 * x + 1 < ws, down = 2 * y + 1 < hs;            // the block may hang over the grid: zeros beyond it
  for (long long z = blockIdx.y; z < planes; z += gridDim.y) {
    const SRC* s = reinterpret_cast<const SRC*>(pyr + z * plane + src_off) + (size_t)2 * y * ws + 2 * x;
    unsigned v = s[0];
    if (right) v += s[1];
    if (down) v += s[ws];
    if (right && down) v += s[ws + 1];
    reinterpret_cast<u16*>(pyr + z * plane + dst_off)[i] = (u16)v;    // <= 255 * 4^l <= 65280
  }
}

struct DefMatchArgs {
  const u8* pyr;
  u8* dsp;
  size_t pyr_plane, dsp_plane, pyr_off, dsp_off, par_off;             // this level in a pyramid / displacement plane; the parent's
  int h, w, wp, tw, top;                                              // wp: the parent's width; top: l = F, init = 0
  long long planes;                                                   // T nout 2: (t, j, direction)
};

// COST: a cost is <= 25 (255 * 4^l)^2, below 2^32 for l <= 2 (25 * 4080^2 = 416160000) and up to 25 * 65280^2 ~ 1.07e11 at l = 4
template <typename PIX, typename COST>
__global__ __launch_bounds__(DEF_THREADS) void deform_match_kernel(DefMatchArgs g) {
  __shared__ u16 Xs[DEF_XH * DEF_XW];
  __shared__ unsigned Ys[DEF_YH * DEF_YW];                             // a dword each: the shift loop's reads are aligned whatever the shift
  __shared__ unsigned Is[DEF_XH * DEF_XW];
  const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * DEF_STRIP;
  const int ty0 = (blockIdx.x / g.tw) * DEF_TH, tx0 = (blockIdx.x % g.tw) * DEF_TW;
  for (long long z = blockIdx.y; z < g.planes; z += gridDim.y) {       // workgroup-uniform
    const PIX* X = reinterpret_cast<const PIX*>(g.pyr + z * g.pyr_plane + g.pyr_off);          // side = direction
    const PIX* Y = reinterpret_cast<const PIX*>(g.pyr + (z ^ 1) * g.pyr_plane + g.pyr_off);    // the other side
    const unsigned* par = reinterpret_cast<const unsigned*>(g.dsp + z * g.dsp_plane + g.par_off);
    for (int i = threadIdx.x; i < DEF_YH * DEF_YW; i += DEF_THREADS) {
      const int ry = i / DEF_YW, rx = i % DEF_YW;
      const int gy = ty0 - 2 * DEF_R + ry, gx = tx0 - 2 * DEF_R + rx;
      const bool in = gy >= 0 && gy < g.h && gx >= 0 && gx < g.w;
      int iy = 0, ix = 0;
      unsigned yv = 0u;
      if (in) {
        if (!g.top) {
          const unsigned pd = par[(size_t)(gy >> 1) * g.wp + (gx >> 1)];   // gy >> 1 < ceil(h / 2): inside the parent
          iy = 2 * def_dy(pd);
          ix = 2 * def_dx(pd);
        }
        const int sy = gy + iy, sx = gx + ix;
        if (sy >= 0 && sy < g.h && sx >= 0 && sx < g.w) yv = Y[(size_t)sy * g.w + sx];
      }
      Ys[i] = yv;
      if (ry >= DEF_R && ry < DEF_YH - DEF_R && rx >= DEF_R && rx < DEF_YW - DEF_R) {
        const int k = (ry - DEF_R) * DEF_XW + rx - DEF_R;
        Is[k] = def_pack(iy, ix);
        Xs[k] = in ? (u16)X[(size_t)gy * g.w + gx] : (u16)0;
      }
    }
    __syncthreads();
    unsigned xr[DEF_ROWS][5];
#pragma unroll
    for (int r = 0; r < DEF_ROWS; ++r)
#pragma unroll
      for (int c = 0; c < 5; ++c) xr[r][c] = Xs[(ly0 + r) * DEF_XW + lx + c];
    COST best[DEF_STRIP];
    int bk[DEF_STRIP];
#pragma unroll
    for (int i = 0; i < DEF_STRIP; ++i) { best[i] = ~(COST)0; bk[i] = 0; }
#pragma unroll 1
    for (int k = 0; k < 25; ++k) {
      const int sy = DEF_SHIFT[k][0], sx = DEF_SHIFT[k][1];
      // window element (a, b) of the pixel in row i of the strip: X at Xs[ly0 + i + a][lx + b], Y' at Ys[ly0 + i + a + sy + 2][lx + b + sx + 2]
      const unsigned* yp = Ys + (ly0 + sy + DEF_R) * DEF_YW + lx + sx + DEF_R;
      COST hsum[DEF_ROWS];
#pragma unroll
      for (int r = 0; r < DEF_ROWS; ++r) {
        COST acc = 0;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
          const unsigned a = xr[r][c], b = yp[r * DEF_YW + c];
          if constexpr (sizeof(COST) == 4) {
            const int d = (int)a - (int)b;                            // l <= 2: |d| <= 4080, one 24-bit multiply-add
            acc += (unsigned)__mul24(d, d);
          } else {
            const unsigned d = a > b ? a - b : b - a;                 // <= 65280: d * d < 2^32
            acc += (COST)d * d;
          }
        }
        hsum[r] = acc;
      }
      COST run = hsum[0] + hsum[1] + hsum[2] + hsum[3] + hsum[4];
#pragma unroll
      for (int i = 0; i < DEF_STRIP; ++i) {
        if (run < best[i]) { best[i] = run; bk[i] = k; }              // strict: the first of equal costs stays
        if (i + 1 < DEF_STRIP) run = run + hsum[i + 5] - hsum[i];
      }
    }
    unsigned* out = reinterpret_cast<unsigned*>(g.dsp + z * g.dsp_plane + g.dsp_off);
#pragma unroll
    for (int i = 0; i < DEF_STRIP; ++i) {
      const int gy = ty0 + ly0 + i, gx = tx0 + lx;
      if (gy < g.h && gx < g.w) {
        const int sy = DEF_SHIFT[bk[i]][0], sx = DEF_SHIFT[bk[i]][1];
        const unsigned iv = Is[(ly0 + i + DEF_R + sy) * DEF_XW + lx + DEF_R + sx];           // init[p + s], 0 outside the grid
        out[(size_t)gy * g.w + gx] = def_pack(sy + def_dy(iv), sx + def_dx(iv));
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ u64 def_shfl_xor_u64(u64 v, int o) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}

struct DefSumArgs {
  const u8* pyr;
  const u8* dsp;
  size_t pyr_plane, dsp_plane;
  int H, W, T, nout, D;
  u64* disp;                                                          // [nout][2][(2 D + 1)^2]
  u64* scalars;                                                       // [nout][2][5]
};

__global__ __launch_bounds__(256) void deform_sums_kernel(DefSumArgs g) {
  extern __shared__ unsigned table[];                                 // (2 D + 1)^2 counts; a workgroup sees <= T P <= 2^31 pixels
  __shared__ u64 red[4][DG_DEFORM_SCALARS];
  const int side = 2 * g.D + 1, nb = side * side;
  const int jd = blockIdx.y, j = jd >> 1, dir = jd & 1;
  const int P = g.H * g.W;
  for (int i = threadIdx.x; i < nb; i += 256) table[i] = 0u;
  __syncthreads();
  u64 acc[DG_DEFORM_SCALARS] = {0ull, 0ull, 0ull, 0ull, 0ull};
  for (int t = 0; t < g.T; ++t) {
    const size_t z = ((size_t)t * g.nout + j) * 2 + dir;
    const u8* X = g.pyr + z * g.pyr_plane;
    const u8* Y = g.pyr + (z ^ 1) * g.pyr_plane;
    const unsigned* d0 = reinterpret_cast<const unsigned*>(g.dsp + z * g.dsp_plane);
    for (int p = blockIdx.x * 256 + threadIdx.x; p < P; p += gridDim.x * 256) {
      const unsigned x = X[p], y = Y[p], dv = d0[p];
      const int dy = def_dy(dv), dx = def_dx(dv);
      const int sy = p / g.W + dy, sx = p % g.W + dx;
      const unsigned m = sy >= 0 && sy < g.H && sx >= 0 && sx < g.W ? Y[(size_t)sy * g.W + sx] : 0u;
      const unsigned em = x > m ? x - m : m - x, er = x > y ? x - y : y - x;
      if (x) {
        const int bin = (dy + g.D) * side + dx + g.D;
        if (dy >= -g.D && dy <= g.D && dx >= -g.D && dx <= g.D) atomicAdd(&table[bin], 1u);   // always: |d_0| <= D by construction
      }
      acc[0] += x ? 1u : 0u;
      acc[1] += (x | m) ? 1u : 0u;
      acc[2] += em * em;
      acc[3] += er * er;
      acc[4] += x * x;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < DG_DEFORM_SCALARS; ++e) {
    u64 v = acc[e];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += def_shfl_xor_u64(v, o);
    if (lane == 0) red[wave][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < DG_DEFORM_SCALARS) {
    const u64 v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (v) atomicAdd(g.scalars + (size_t)jd * DG_DEFORM_SCALARS + threadIdx.x, v);
  }
  for (int i = threadIdx.x; i < nb; i += 256) {
    const unsigned v = table[i];
    if (v) atomicAdd(g.disp + (size_t)jd * nb + i, (u64)v);
  }
}

__global__ __launch_bounds__(256) void deform_emit_kernel(const u8* pyr, const u8* dsp, size_t pyr_plane, size_t dsp_plane, int H, int W,
                                                          long long planes, short* field, u8* morphed) {
  const int P = H * W, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  for (long long z = blockIdx.y; z < planes; z += gridDim.y) {
    const unsigned dv = reinterpret_cast<const unsigned*>(dsp + z * dsp_plane)[p];
    const int dy = def_dy(dv), dx = def_dx(dv);
    field[(z * 2 + 0) * P + p] = (short)dy;
    field[(z * 2 + 1) * P + p] = (short)dx;
    if (morphed) {
      const u8* Y = pyr + (z ^ 1) * pyr_plane;
      const int sy = p / W + dy, sx = p % W + dx;
      morphed[z * P + p] = sy >= 0 && sy < H && sx >= 0 && sx < W ? Y[(size_t)sy * W + sx] : (u8)0;
    }
  }
}

bool grid_ok(int H, int W) { return H >= 1 && W >= 1 && H <= DG_DEFORM_MAX_SIDE && W <= DG_DEFORM_MAX_SIDE; }

int max_disp(int F) { return 2 * ((2 << F) - 1); }                    // D = 2 (2^(F+1) - 1)

bool spec_ok(const dg_deform_spec* s, int C) {
  if (!s || s->levels < 1 || s->levels > MAXL || !hist_xform_ok(s, C)) return false;
  for (int j = 0; j < hist_nout(s, C); ++j)
    if (!hist_finite(s->lo[j]) || !hist_finite(s->inv_step[j]) || !(s->inv_step[j] > 0.f)) return false;
  return true;
}

inline size_t round16(size_t n) { return (n + 15) / 16 * 16; }

struct Layout {
  int nout, F, D, nb;
  int h[MAXL + 1], w[MAXL + 1];
  size_t pyr_off[MAXL + 1], dsp_off[MAXL + 1];                        // bytes of level l inside one plane
  size_t pyr_plane, dsp_plane;                                        // bytes of one (t, j, side) pyramid / (t, j, direction) displacement set
  size_t pyr_bytes, bytes;
};

Layout layout_of(int T, int C, int H, int W, const dg_deform_spec* s) {
  Layout l;
  l.nout = hist_nout(s, C);
  l.F = s->levels;
  l.D = max_disp(l.F);
  l.nb = (2 * l.D + 1) * (2 * l.D + 1);
  size_t po = 0, dof = 0;
  for (int k = 0; k <= l.F; ++k) {
    l.h[k] = (H + (1 << k) - 1) >> k;
    l.w[k] = (W + (1 << k) - 1) >> k;
    const size_t n = (size_t)l.h[k] * l.w[k];
    l.pyr_off[k] = po;
    l.dsp_off[k] = dof;
    po += round16(n * (k == 0 ? 1 : 2));                              // level 0 uint8, above uint16
    dof += round16(n * 4);                                            // (dy, dx) int16
  }
  l.pyr_plane = po;
  l.dsp_plane = dof;
  const size_t planes = (size_t)T * l.nout * 2;
  l.pyr_bytes = hist_round256(planes * l.pyr_plane);
  l.bytes = l.pyr_bytes + hist_round256(planes * l.dsp_plane);
  return l;
}

bool call_ok(const dg_eof_fields* a, int H, int W, const dg_deform_spec* s) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C)) return false;
  if (!grid_ok(H, W) || (long long)H * W != a->P) return false;
  if ((long long)a->T * a->P > DEF_PIX_LIMIT) return false;           // the uint32 LDS counts of a workgroup
  return a->T <= DEF_LIMIT / (DEF_FIELD_MAX * a->P);                  // T * bound <= 2^62: one call cannot overflow
}

// everything up to d_0 of both directions of every (t, j) in the workspace
int run_matcher(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_deform_spec* s, void* ws, const Layout& l,
                hipStream_t st) {
  u8* pyr = reinterpret_cast<u8*>(ws);
  u8* dsp = pyr + l.pyr_bytes;
  const long long planes = (long long)a->T * l.nout * 2;
  const unsigned gz = (unsigned)(planes < DEF_GRID_Z ? planes : DEF_GRID_Z);
  const dg_eof_fields* series[2] = {a, b};
  for (int side = 0; side < 2; ++side) {
    DefQuantArgs q;
    q.x = hist_series(series[side]);
    q.xf = hist_xform(s, a->C);
    q.P = a->P; q.T = a->T; q.nout = l.nout; q.side = side;
    for (int j = 0; j < MAXO; ++j) { q.lo[j] = j < l.nout ? s->lo[j] : 0.f; q.inv_step[j] = j < l.nout ? s->inv_step[j] : 1.f; }
    q.pyr = pyr; q.plane = l.pyr_plane;
    const dim3 grid((unsigned)((a->P + 255) / 256), (unsigned)(a->T < DEF_GRID_Z ? a->T : DEF_GRID_Z));
    hist_dispatch<false>(series[side]->dtype, hist_mode(series[side]), [&](auto t, auto m) {
      hipLaunchKernelGGL((deform_quant_kernel<decltype(t), decltype(m)::value>), grid, dim3(256), 0, st, q);
    });
  }
  for (int k = 1; k <= l.F; ++k) {
    const dim3 grid((unsigned)((l.h[k] * l.w[k] + 255) / 256), gz);
    if (k == 1)
      hipLaunchKernelGGL(deform_down_kernel<u8>, grid, dim3(256), 0, st, pyr, l.pyr_plane, l.pyr_off[0], l.pyr_off[1], l.h[0], l.w[0],
                         l.h[1], l.w[1], planes);
    else
      hipLaunchKernelGGL(deform_down_kernel<u16>, grid, dim3(256), 0, st, pyr, l.pyr_plane, l.pyr_off[k - 1], l.pyr_off[k], l.h[k - 1],
                         l.w[k - 1], l.h[k], l.w[k], planes);
  }
  for (int k = l.F; k >= 0; --k) {
    DefMatchArgs m;
    m.pyr = pyr; m.dsp = dsp;
    m.pyr_plane = l.pyr_plane; m.dsp_plane = l.dsp_plane;
    m.pyr_off = l.pyr_off[k]; m.dsp_off = l.dsp_off[k];
    m.top = k == l.F;
    m.par_off = m.top ? 0 : l.dsp_off[k + 1];
    m.h = l.h[k]; m.w = l.w[k];
    m.wp = m.top ? 0 : l.w[k + 1];
    m.tw = (m.w + DEF_TW - 1) / DEF_TW;
    m.planes = planes;
    const dim3 grid((unsigned)(m.tw * ((m.h + DEF_TH - 1) / DEF_TH)), gz);
    if (k == 0)
      hipLaunchKernelGGL((deform_match_kernel<u8, unsigned>), grid, dim3(DEF_THREADS), 0, st, m);
    else if (k <= 2)
      hipLaunchKernelGGL((deform_match_kernel<u16, unsigned>), grid, dim3(DEF_THREADS), 0, st, m);
    else
      hipLaunchKernelGGL((deform_match_kernel<u16, u64>), grid, dim3(DEF_THREADS), 0, st, m);
  }
  return dg_check_launch();
}

bool pair_ok(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_deform_spec* s) {
  return call_ok(a, H, W, s) && hist_fields_ok(b) && b->T == a->T && b->C == a->C && b->P == a->P;
}

bool dtypes_ok(const dg_eof_fields* a, const dg_eof_fields* b) {
  return (a->dtype == DG_F32 || a->dtype == DG_BF16) && (b->dtype == DG_F32 || b->dtype == DG_BF16);
}

// ---- the host reference: the definition by plain loops, independent of the kernels' separable form ---------------------------------

struct HostShift { int sy, sx; };

std::vector<HostShift> host_shifts() {
  std::vector<HostShift> v;
  for (int sy = -2; sy <= 2; ++sy)
    for (int sx = -2; sx <= 2; ++sx) v.push_back({sy, sx});
  std::stable_sort(v.begin(), v.end(), [](const HostShift& p, const HostShift& q) {
    const int rp = p.sy * p.sy + p.sx * p.sx, rq = q.sy * q.sy + q.sx * q.sx;
    if (rp != rq) return rp < rq;
    if (p.sy != q.sy) return p.sy < q.sy;
    return p.sx < q.sx;
  });
  return v;
}

struct HostPlane {
  int h, w;
  std::vector<int64_t> v;
  int64_t at(int y, int x) const { return y >= 0 && y < h && x >= 0 && x < w ? v[(size_t)y * w + x] : 0; }
};

std::vector<HostPlane> host_pyramid(const dg_deform_spec* s, const float* x, int C, int H, int W, int j) {
  std::vector<HostPlane> pyr(s->levels + 1);
  pyr[0].h = H; pyr[0].w = W;
  pyr[0].v.resize((size_t)H * W);
  const size_t P = (size_t)H * W;
  for (size_t p = 0; p < P; ++p) pyr[0].v[p] = def_quant(hist_host_value(s, x, C, P, p, j), s->lo[j], s->inv_step[j]);
  for (int l = 1; l <= s->levels; ++l) {
    const HostPlane& src = pyr[l - 1];
    HostPlane& dst = pyr[l];
    dst.h = (src.h + 1) / 2; dst.w = (src.w + 1) / 2;
    dst.v.resize((size_t)dst.h * dst.w);
    for (int y = 0; y < dst.h; ++y)
      for (int xx = 0; xx < dst.w; ++xx)
        dst.v[(size_t)y * dst.w + xx] = src.at(2 * y, 2 * xx) + src.at(2 * y, 2 * xx + 1) + src.at(2 * y + 1, 2 * xx) + src.at(2 * y + 1, 2 * xx + 1);
  }
  return pyr;
}

struct HostDisp {
  int h, w;
  std::vector<int> dy, dx;
};

// d_0 of target pyramid X, source pyramid Y
HostDisp host_match(const std::vector<HostPlane>& X, const std::vector<HostPlane>& Y, int F) {
  const std::vector<HostShift> shifts = host_shifts();
  HostDisp par;
  par.h = par.w = 0;
  for (int l = F; l >= 0; --l) {
    const int h = X[l].h, w = X[l].w;
    HostPlane iy, ix, yp;                                             // init and Y' on the level's grid, 0 outside
    iy.h = ix.h = yp.h = h; iy.w = ix.w = yp.w = w;
    iy.v.assign((size_t)h * w, 0); ix.v.assign((size_t)h * w, 0); yp.v.assign((size_t)h * w, 0);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const size_t p = (size_t)y * w + x;
        if (l < F) {
          iy.v[p] = 2 * par.dy[(size_t)(y >> 1) * par.w + (x >> 1)];
          ix.v[p] = 2 * par.dx[(size_t)(y >> 1) * par.w + (x >> 1)];
        }
        yp.v[p] = Y[l].at(y + (int)iy.v[p], x + (int)ix.v[p]);
      }
    HostDisp cur;
    cur.h = h; cur.w = w;
    cur.dy.resize((size_t)h * w); cur.dx.resize((size_t)h * w);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        int64_t best = -1;
        HostShift bs{0, 0};
        for (const HostShift& sh : shifts) {
          int64_t cost = 0;                                           // <= 25 * 65280^2: int64
          for (int wy = -2; wy <= 2; ++wy)
            for (int wx = -2; wx <= 2; ++wx) {
              const int64_t d = X[l].at(y + wy, x + wx) - yp.at(y + wy + sh.sy, x + wx + sh.sx);
              cost += d * d;
            }
          if (best < 0 || cost < best) { best = cost; bs = sh; }
        }
        cur.dy[(size_t)y * w + x] = bs.sy + (int)iy.at(y + bs.sy, x + bs.sx);
        cur.dx[(size_t)y * w + x] = bs.sx + (int)ix.at(y + bs.sy, x + bs.sx);
      }
    par = cur;
  }
  return par;
}

int host_run(const dg_deform_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* disp, int64_t* scalars, int16_t* field,
             uint8_t* morphed) {
  if (!spec_ok(s, C) || !a || !b || !grid_ok(H, W)) return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C), F = s->levels, D = max_disp(F), side = 2 * D + 1;
  const size_t P = (size_t)H * W;
  for (int j = 0; j < nout; ++j) {
    const std::vector<HostPlane> pa = host_pyramid(s, a, C, H, W, j), pb = host_pyramid(s, b, C, H, W, j);
    for (int dir = 0; dir < 2; ++dir) {
      const std::vector<HostPlane>& X = dir ? pb : pa;
      const std::vector<HostPlane>& Y = dir ? pa : pb;
      const HostDisp d = host_match(X, Y, F);
      const size_t jd = (size_t)j * 2 + dir;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const size_t p = (size_t)y * W + x;
          const int dy = d.dy[p], dx = d.dx[p];
          const int64_t xv = X[0].v[p], yv = Y[0].v[p], m = Y[0].at(y + dy, x + dx);
          if (field) {
            field[(jd * 2 + 0) * P + p] = (int16_t)dy;
            field[(jd * 2 + 1) * P + p] = (int16_t)dx;
          }
          if (morphed) morphed[jd * P + p] = (uint8_t)m;
          if (disp && xv > 0) {
            if (dy < -D || dy > D || dx < -D || dx > D) return DG_ERR_BAD_ARG;   // cannot happen: |d_0| <= D
            disp[jd * side * side + (size_t)(dy + D) * side + dx + D] += 1;
          }
          if (scalars) {
            int64_t* o = scalars + jd * DG_DEFORM_SCALARS;
            o[0] += xv > 0;
            o[1] += xv > 0 || m > 0;
            o[2] += (xv - m) * (xv - m);
            o[3] += (xv - yv) * (xv - yv);
            o[4] += xv * xv;
          }
        }
    }
  }
  return DG_OK;
}

}  // namespace

extern "C" int64_t dg_deform_bound(int H, int W) { return grid_ok(H, W) ? DEF_FIELD_MAX * H * W : 0; }

extern "C" size_t dg_deform_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_deform_spec* s) {
  if (!call_ok(a, H, W, s)) return 0;
  return layout_of(a->T, a->C, H, W, s).bytes;
}

extern "C" int dg_deform_host(const dg_deform_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* disp, int64_t* scalars) {
  if (!disp || !scalars) return DG_ERR_BAD_SHAPE;
  return host_run(s, a, b, C, H, W, disp, scalars, nullptr, nullptr);
}

extern "C" int dg_deform_field_host(const dg_deform_spec* s, const float* a, const float* b, int C, int H, int W, int16_t* field,
                                    uint8_t* morphed) {
  if (!field) return DG_ERR_BAD_SHAPE;
  return host_run(s, a, b, C, H, W, nullptr, nullptr, field, morphed);
}

extern "C" int dg_deform(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_deform_spec* s, void* ws, int64_t* disp,
                         int64_t* scalars, void* stream) {
  if (!pair_ok(a, b, H, W, s) || !ws || !disp || !scalars) return DG_ERR_BAD_SHAPE;
  if (!dtypes_ok(a, b)) return DG_ERR_BAD_DTYPE;
  const Layout l = layout_of(a->T, a->C, H, W, s);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = run_matcher(a, b, H, W, s, ws, l, st);
  if (rc != DG_OK) return rc;
  DefSumArgs g;
  g.pyr = reinterpret_cast<const u8*>(ws);
  g.dsp = g.pyr + l.pyr_bytes;
  g.pyr_plane = l.pyr_plane; g.dsp_plane = l.dsp_plane;
  g.H = H; g.W = W; g.T = a->T; g.nout = l.nout; g.D = l.D;
  g.disp = reinterpret_cast<u64*>(disp);
  g.scalars = reinterpret_cast<u64*>(scalars);
  // few, fat workgroups: each flushes its whole table once
  const int blocks = (a->P + 255) / 256, most = 2048 / (l.nout * 2) > 1 ? 2048 / (l.nout * 2) : 1;
  const dim3 grid((unsigned)(blocks < most ? blocks : most), (unsigned)(l.nout * 2));
  hipLaunchKernelGGL(deform_sums_kernel, grid, dim3(256), (size_t)l.nb * sizeof(unsigned), st, g);
  return dg_check_launch();
}

extern "C" int dg_deform_field(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_deform_spec* s, void* ws,
                               int16_t* field, uint8_t* morphed, void* stream) {
  if (!pair_ok(a, b, H, W, s) || !ws || !field) return DG_ERR_BAD_SHAPE;
  if (!dtypes_ok(a, b)) return DG_ERR_BAD_DTYPE;
  const Layout l = layout_of(a->T, a->C, H, W, s);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = run_matcher(a, b, H, W, s, ws, l, st);
  if (rc != DG_OK) return rc;
  const long long planes = (long long)a->T * l.nout * 2;
  const u8* pyr = reinterpret_cast<const u8*>(ws);
  const dim3 grid((unsigned)((a->P + 255) / 256), (unsigned)(planes < DEF_GRID_Z ? planes : DEF_GRID_Z));
  hipLaunchKernelGGL(deform_emit_kernel, grid, dim3(256), 0, st, pyr, pyr + l.pyr_bytes, l.pyr_plane, l.dsp_plane, H, W, planes,
                     reinterpret_cast<short*>(field), reinterpret_cast<u8*>(morphed));
  return dg_check_launch();
}
