// Intensity-scale verification (include/downgan_hip.h "Intensity-scale verification") of two series of H x W fields read through the
// EOF descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16): for every output channel j, threshold k and level l = 0 .. n
// (2^n >= max(H, W)) the exact integers D_l = sum (S_b - S_a)^2, A_l = sum S_a^2, B_l = sum S_b^2 of the sums of the exceedance
// masks over the aligned blocks of side 2^l of the zero-padded 2^n x 2^n square.
//   iscale_tiles_kernel<TA, MA, TB, MB>  one workgroup of four waves per 64 x 64 tile of one field pair.  A wave takes 16 rows of the
//                              tile: per row 64 pixels of both series (the loads of four rows issued together), the output
//                              values y of hist_common.h, the masks of all (j, k) as wave ballots -> one 64-bit word per (j, k),
//                              side and row in LDS.  Then the (j, k) are dealt to the waves, lane r takes the words of row r: level 0 by
//                              popcounts; levels 1 .. 6 by packed counts (the popcount ladder, halted at each level) added down the
//                              2^l rows of a block by one xor shuffle per level; the fields squared and summed in 32 bits (a tile
//                              adds at most 4^(6+l) <= 2^24 to a level), reduced over the block rows by xor shuffles, one 64-bit
//                              integer atomic per (level, term) into the field's slot.  The tile totals (<= 4096 each, 16 bits a
//                              side) go to the workspace when n > 6
//   iscale_pyramid_kernel      n > 6 only; workgroup = one (t, j, k): the totals of the <= 32 x 32 tiles in LDS (zero where the
//                              padded square has no tile), halved per level 7 .. n; squares in 64-bit, wave shuffles, LDS over the
//                              waves, a plain store into the slot (nobody else writes these levels)
//   iscale_finish_kernel       sums += the slots over t (and the slots copied to per_field)
// MA, MB: HIST_PIX16 = one 16-byte load per pixel (the generator's [B, H, W, 16] bf16 output), HIST_ANY = one element per load
// (NCHW planes too: a wave's 64 pixels are consecutive, so the loads coalesce).  Every pixel of each series is read once, nothing
// per pixel is written; no float after the compare, integer atomics only: exact, and two calls on the same data are bit-identical.
#include <float.h>
#include <math.h>

#include <vector>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

constexpr int ISC_TILE = 64;                          // the tile side: the lanes of a ballot, and of the second phase's rows
constexpr int ISC_TILE_LOG = 6;
constexpr int ISC_WAVES = 4, ISC_THREADS = ISC_WAVES * 64;            // the waves of a workgroup share its tile
constexpr int ISC_WAVE_ROWS = ISC_TILE / ISC_WAVES;   // rows of the tile a wave turns into words
constexpr int ISC_ROWS = 4;                           // of them in flight at a time: the row walk is a chain of load latencies
static_assert(ISC_WAVE_ROWS % ISC_ROWS == 0, "whole groups of rows");
constexpr int ISC_LDS_MAX = 64 * 1024;                // words of a tile: 1 KiB per (j, k)
constexpr int ISC_PYR_THREADS = 256;
constexpr int ISC_PYR_WAVES = ISC_PYR_THREADS / 64;
constexpr int ISC_MAX_TILES = DG_ISCALE_MAX_SIDE / ISC_TILE;          // per side
constexpr int ISC_GRID_T = 4096;                      // fields across gridDim.y at most; the kernels stride over the rest
constexpr int MAXO = DG_HIST_MAX_OUT, MAXK = DG_ISCALE_MAX_THR;
constexpr long long ISC_LIMIT = 1LL << 62;
static_assert(DG_ISCALE_MAX_SIDE == ISC_TILE << (DG_ISCALE_MAX_LEVELS - 1 - ISC_TILE_LOG), "levels of the largest grid");
static_assert(MAXO * MAXK * 2 * ISC_TILE * 8 <= ISC_LDS_MAX, "a tile's words fit");

typedef unsigned long long u64;

struct IscTileArgs {
  HistSeries a, b;
  HistXform xf;
  int H, W, T, nout, nthr, n, tw, ntiles;             // tw: tiles per row of tiles; ntiles = tiles of one field (real ones only)
  float thr[MAXO][MAXK];
  u64* slots;                                         // [T][nout][nthr][n + 1][3]
  unsigned* totals;                                   // [T][nout][nthr][ntiles]: S_6(I_a) | S_6(I_b) << 16
};

struct IscPyrArgs {
  const unsigned* totals;
  u64* slots;
  int T, njk, n, th, tw;
};

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}

// The block sums of the levels 1 .. 6 that the row word x of this lane (= row) lies in, packed: level l as 64 / 2^l fields, one per
// block column.  Levels 1 and 2 need one bit more than their 2^l-bit field, so they are held as the even and the odd block columns
// in fields of twice the width.  Every lane of a block row ends with the same words.
struct IscLevels {
  u64 e1, o1;                 // 16 + 16 fields of 4 bits, <= 4
  u64 e2, o2;                 // 8 + 8 fields of 8 bits, <= 16
  u64 v3, v4, v5, v6;         // 8 x 8 bits <= 64, 4 x 16 bits <= 256, 2 x 32 bits <= 1024, 1 x 64 bits <= 4096
};

__device__ __forceinline__ IscLevels isc_levels(u64 x) {
  IscLevels p;
  const u64 c1 = x - ((x >> 1) & 0x5555555555555555ull);             // 1 row x 2 columns, <= 2
  u64 e = c1 & 0x3333333333333333ull, o = (c1 >> 2) & 0x3333333333333333ull;
  e += shfl_xor_u64(e, 1); o += shfl_xor_u64(o, 1);                  // 2 x 2
  p.e1 = e; p.o1 = o;
  const u64 h2 = e + o;                                              // 2 rows x 4 columns in 4 bits, <= 8
  e = h2 & 0x0f0f0f0f0f0f0f0full; o = (h2 >> 4) & 0x0f0f0f0f0f0f0f0full;
  e += shfl_xor_u64(e, 2); o += shfl_xor_u64(o, 2);                  // 4 x 4
  p.e2 = e; p.o2 = o;
  u64 v = e + o;                                                     // 4 rows x 8 columns in 8 bits, <= 32
  v += shfl_xor_u64(v, 4);                                           // 8 x 8
  p.v3 = v;
  v = (v & 0x00ff00ff00ff00ffull) + ((v >> 8) & 0x00ff00ff00ff00ffull);
  v += shfl_xor_u64(v, 8);                                           // 16 x 16
  p.v4 = v;
  v = (v & 0x0000ffff0000ffffull) + ((v >> 16) & 0x0000ffff0000ffffull);
  v += shfl_xor_u64(v, 16);                                          // 32 x 32
  p.v5 = v;
  v = (v & 0xffffffffull) + (v >> 32);
  v += shfl_xor_u64(v, 32);                                          // 64 x 64
  p.v6 = v;
  return p;
}

// acc += (D, A, B) of the 64 / BITS fields of BITS bits of the two sides' words
template <int BITS>
__device__ __forceinline__ void isc_squares(u64 wa, u64 wb, unsigned (&acc)[3]) {
  const u64 m = BITS == 64 ? ~0ull : (1ull << (BITS & 63)) - 1ull;
#pragma unroll
  for (int f = 0; f < 64 / BITS; ++f) {
    const unsigned ca = (unsigned)((wa >> (f * BITS)) & m), cb = (unsigned)((wb >> (f * BITS)) & m);
    const unsigned d = ca > cb ? ca - cb : cb - ca;
    acc[0] += d * d;
    acc[1] += ca * ca;
    acc[2] += cb * cb;
  }
}

template <typename TA, int MA, typename TB, int MB>
__global__ __launch_bounds__(ISC_THREADS) void iscale_tiles_kernel(IscTileArgs g) {
  extern __shared__ __attribute__((aligned(16))) u64 words[];        // [(j, k)][side][row] of the workgroup's tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int njk = g.nout * g.nthr, nlev = g.n + 1;
  const int tile = blockIdx.x;
  const int h0 = (tile / g.tw) * ISC_TILE, w0 = (tile % g.tw) * ISC_TILE;
  const int rows = g.H - h0 < ISC_TILE ? g.H - h0 : ISC_TILE;
  const int w = w0 + lane;
  const bool in = w < g.W;
  const TA* abase = reinterpret_cast<const TA*>(g.a.base);
  const TB* bbase = reinterpret_cast<const TB*>(g.b.base);
  for (int t = blockIdx.y; t < g.T; t += gridDim.y) {               // workgroup-uniform
    // wave q takes the rows q * 16 .. q * 16 + 15 of the tile, ISC_ROWS at a time: their loads are issued before their ballots
    for (int r0 = wave * ISC_WAVE_ROWS; r0 < (wave + 1) * ISC_WAVE_ROWS; r0 += ISC_ROWS) {
      if (r0 >= rows) {                                              // wave-uniform: rows below the grid are empty
        for (int i = lane; i < njk * 2 * ISC_ROWS; i += 64) words[(i / ISC_ROWS) * ISC_TILE + r0 + i % ISC_ROWS] = 0ull;
        continue;
      }
      HistPixelRaw<MA> ra[ISC_ROWS];
      HistPixelRaw<MB> rb[ISC_ROWS];
#pragma unroll
      for (int u = 0; u < ISC_ROWS; ++u) {
        const int h = h0 + (r0 + u < rows ? r0 + u : rows - 1);      // rows past the tile's last read it again, unused
        const long long p = (long long)h * g.W + (in ? w : g.W - 1); // lanes beyond the row read its last pixel, unused
        hist_pixel_load<TA, MA>(g.xf, abase + t * g.a.ld_t + p * g.a.ld_p, g.a.ld_c, ra[u]);
        hist_pixel_load<TB, MB>(g.xf, bbase + t * g.b.ld_t + p * g.b.ld_p, g.b.ld_c, rb[u]);
      }
#pragma unroll
      for (int u = 0; u < ISC_ROWS; ++u) {
        const bool on = in && r0 + u < rows;
        float ya[MAXO], yb[MAXO];
        hist_pixel_finish<TA, MA>(g.xf, ra[u], ya);
        hist_pixel_finish<TB, MB>(g.xf, rb[u], yb);
#pragma unroll
        for (int j = 0; j < MAXO; ++j) {
          if (j < g.nout) {
#pragma unroll
            for (int k = 0; k < MAXK; ++k) {
              if (k < g.nthr) {
                const u64 ma = __ballot(on && ya[j] > g.thr[j][k]), mb = __ballot(on && yb[j] > g.thr[j][k]);
                if (lane == 0) {
                  u64* q = words + (size_t)(j * g.nthr + k) * 2 * ISC_TILE + r0 + u;
                  q[0] = ma;
                  q[ISC_TILE] = mb;
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    {
      for (int jk = wave; jk < njk; jk += ISC_WAVES) {             // wave-uniform: the (j, k) are dealt to the waves
        const u64 xa = words[(size_t)jk * 2 * ISC_TILE + lane], xb = words[(size_t)jk * 2 * ISC_TILE + ISC_TILE + lane];
        unsigned s[ISC_TILE_LOG + 1][3];
#pragma unroll
        for (int l = 0; l <= ISC_TILE_LOG; ++l) s[l][0] = s[l][1] = s[l][2] = 0u;
        s[0][0] = (unsigned)__popcll(xa ^ xb);
        s[0][1] = (unsigned)__popcll(xa);
        s[0][2] = (unsigned)__popcll(xb);
        const IscLevels pa = isc_levels(xa), pb = isc_levels(xb);
        isc_squares<4>(pa.e1, pb.e1, s[1]); isc_squares<4>(pa.o1, pb.o1, s[1]);
        isc_squares<8>(pa.e2, pb.e2, s[2]); isc_squares<8>(pa.o2, pb.o2, s[2]);
        isc_squares<8>(pa.v3, pb.v3, s[3]);
        isc_squares<16>(pa.v4, pb.v4, s[4]);
        isc_squares<32>(pa.v5, pb.v5, s[5]);
        isc_squares<64>(pa.v6, pb.v6, s[6]);
        // the lanes of a block row hold the same sums: add over the block rows only, 6 - l steps at level l
        unsigned out = 0u;
#pragma unroll
        for (int l = 0; l <= ISC_TILE_LOG; ++l) {
#pragma unroll
          for (int e = 0; e < 3; ++e) {
            unsigned v = s[l][e];
#pragma unroll
            for (int o = 1 << l; o <= 32; o <<= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
            out = lane == l * 3 + e ? v : out;
          }
        }
        const int l = lane / 3, e = lane % 3;
        if (l < nlev && l <= ISC_TILE_LOG && out)
          atomicAdd(g.slots + (((long long)t * njk + jk) * nlev + l) * 3 + e, (u64)out);
        if (g.n > ISC_TILE_LOG && lane == 0)
          g.totals[((long long)t * njk + jk) * g.ntiles + tile] = (unsigned)pa.v6 | ((unsigned)pb.v6 << 16);
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += shfl_xor_u64(v, o);
  return v;
}

__global__ __launch_bounds__(ISC_PYR_THREADS) void iscale_pyramid_kernel(IscPyrArgs g) {
  __shared__ int cnt[2][2][ISC_MAX_TILES * ISC_MAX_TILES];           // [buffer][side][block]: the second buffer holds a quarter
  __shared__ u64 red[ISC_PYR_WAVES][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jk = blockIdx.x, nlev = g.n + 1, side0 = 1 << (g.n - ISC_TILE_LOG);
  for (int t = blockIdx.y; t < g.T; t += gridDim.y) {               // workgroup-uniform
    const unsigned* tot = g.totals + ((long long)t * g.njk + jk) * g.th * g.tw;
    for (int i = threadIdx.x; i < side0 * side0; i += ISC_PYR_THREADS) {
      const int ty = i / side0, tx = i % side0;
      const unsigned v = ty < g.th && tx < g.tw ? tot[ty * g.tw + tx] : 0u;   // no tile: an empty part of the padded square
      cnt[0][0][i] = (int)(v & 0xffffu);
      cnt[0][1][i] = (int)(v >> 16);
    }
    __syncthreads();
    int src = 0, side = side0;
    for (int l = ISC_TILE_LOG + 1; l <= g.n; ++l) {
      const int m = side >> 1;
      u64 acc[3] = {0ull, 0ull, 0ull};
      for (int i = threadIdx.x; i < m * m; i += ISC_PYR_THREADS) {
        const int y = i / m, x = i % m, q = 2 * y * side + 2 * x;
        const int* sa = cnt[src][0];
        const int* sb = cnt[src][1];
        const int ca = sa[q] + sa[q + 1] + sa[q + side] + sa[q + side + 1];
        const int cb = sb[q] + sb[q + 1] + sb[q + side] + sb[q + side + 1];
        cnt[src ^ 1][0][i] = ca;
        cnt[src ^ 1][1][i] = cb;
        const u64 ua = (u64)ca, ub = (u64)cb, d = ua > ub ? ua - ub : ub - ua;
        acc[0] += d * d;
        acc[1] += ua * ua;
        acc[2] += ub * ub;
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const u64 v = wave_sum_u64(acc[e]);
        if (lane == 0) red[wave][e] = v;
      }
      __syncthreads();
      if (threadIdx.x < 3) {
        u64 v = 0ull;
        for (int q = 0; q < ISC_PYR_WAVES; ++q) v += red[q][threadIdx.x];
        g.slots[(((long long)t * g.njk + jk) * nlev + l) * 3 + threadIdx.x] = v;
      }
      __syncthreads();
      src ^= 1;
      side = m;
    }
  }
}

__global__ __launch_bounds__(256) void iscale_finish_kernel(const u64* slots, int T, int n, u64* sums, u64* per_field) {
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    u64 total = 0ull;
    for (int t = 0; t < T; ++t) {
      const u64 v = slots[(long long)t * n + i];
      total += v;
      if (per_field) per_field[(long long)t * n + i] = v;
    }
    sums[i] += total;
  }
}

bool grid_ok(int H, int W) { return H >= 1 && W >= 1 && H <= DG_ISCALE_MAX_SIDE && W <= DG_ISCALE_MAX_SIDE; }

// n: the smallest integer with 2^n >= max(H, W)
int log_side(int H, int W) {
  const int m = H > W ? H : W;
  int n = 0;
  while ((1 << n) < m) ++n;
  return n;
}

bool spec_ok(const dg_iscale_spec* s, int C) {
  if (!s || s->nthr < 1 || s->nthr > MAXK) return false;
  return hist_xform_ok(s, C) && hist_thr_ok(s->thr, hist_nout(s, C), s->nthr);
}

struct Layout {
  int nout, njk, n, th, tw;
  size_t slot_bytes, bytes;
};

Layout layout_of(const dg_eof_fields* a, int H, int W, const dg_iscale_spec* s) {
  Layout l;
  l.nout = hist_nout(s, a->C);
  l.njk = l.nout * s->nthr;
  l.n = log_side(H, W);
  l.th = (H + ISC_TILE - 1) / ISC_TILE;
  l.tw = (W + ISC_TILE - 1) / ISC_TILE;
  l.slot_bytes = hist_round256((size_t)a->T * l.njk * (l.n + 1) * 3 * sizeof(u64));
  l.bytes = l.slot_bytes + hist_round256((size_t)a->T * l.njk * l.th * l.tw * sizeof(unsigned));
  return l;
}

bool call_ok(const dg_eof_fields* a, int H, int W, const dg_iscale_spec* s) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C)) return false;
  if (!grid_ok(H, W) || (long long)H * W != a->P) return false;
  return a->T <= ISC_LIMIT >> (4 * log_side(H, W));                  // T * 16^n <= 2^62: one call cannot overflow
}

template <typename TA, int MA>
void tiles_of(const dg_eof_fields* b, const IscTileArgs& g, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  hist_dispatch<false>(b->dtype, hist_mode(b), [&](auto t, auto m) {
    hipLaunchKernelGGL((iscale_tiles_kernel<TA, MA, decltype(t), decltype(m)::value>), grid, block, lds, st, g);
  });
}

}  // namespace

extern "C" int dg_iscale_levels(int H, int W) { return grid_ok(H, W) ? log_side(H, W) + 1 : 0; }

extern "C" int64_t dg_iscale_bound(int H, int W) { return grid_ok(H, W) ? (int64_t)1 << (4 * log_side(H, W)) : 0; }

extern "C" size_t dg_iscale_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_iscale_spec* s) {
  if (!call_ok(a, H, W, s)) return 0;
  return layout_of(a, H, W, s).bytes;
}

extern "C" int dg_iscale_host(const dg_iscale_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* sums) {
  if (!spec_ok(s, C) || !a || !b || !sums || !grid_ok(H, W)) return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C), n = log_side(H, W);
  const size_t P = (size_t)H * W;
  std::vector<unsigned char> mask[2];
  mask[0].resize(P);
  mask[1].resize(P);
  const float* x[2] = {a, b};
  for (int j = 0; j < nout; ++j) {
    for (int k = 0; k < s->nthr; ++k) {
      for (int side = 0; side < 2; ++side)
        for (size_t p = 0; p < P; ++p) mask[side][p] = hist_host_value(s, x[side], C, P, p, j) > s->thr[j][k] ? 1 : 0;
      for (int l = 0; l <= n; ++l) {
        const int64_t bs = (int64_t)1 << l, nb = (int64_t)1 << (n - l);        // block side, blocks per side of the padded square
        int64_t D = 0, A = 0, B = 0;
        for (int64_t by = 0; by < nb && by * bs < H; ++by) {                     // the blocks beyond the grid are empty
          for (int64_t bx = 0; bx < nb && bx * bs < W; ++bx) {
            int64_t c[2] = {0, 0};
            for (int64_t h = by * bs; h < (by + 1) * bs && h < H; ++h)
              for (int64_t w = bx * bs; w < (bx + 1) * bs && w < W; ++w) {
                c[0] += mask[0][(size_t)h * W + w];
                c[1] += mask[1][(size_t)h * W + w];
              }
            D += (c[1] - c[0]) * (c[1] - c[0]);
            A += c[0] * c[0];
            B += c[1] * c[1];
          }
        }
        int64_t* o = sums + ((size_t)(j * s->nthr + k) * (n + 1) + l) * 3;
        o[0] += D; o[1] += A; o[2] += B;
      }
    }
  }
  return DG_OK;
}

extern "C" int dg_iscale(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_iscale_spec* s, void* ws, int64_t* sums,
                         int64_t* per_field, void* stream) {
  if (!call_ok(a, H, W, s) || !hist_fields_ok(b) || b->T != a->T || b->C != a->C || b->P != a->P || !ws || !sums)
    return DG_ERR_BAD_SHAPE;
  if ((a->dtype != DG_F32 && a->dtype != DG_BF16) || (b->dtype != DG_F32 && b->dtype != DG_BF16)) return DG_ERR_BAD_DTYPE;
  const Layout l = layout_of(a, H, W, s);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  u64* slots = reinterpret_cast<u64*>(ws);
  unsigned* totals = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ws) + l.slot_bytes);
  if (hipMemsetAsync(slots, 0, l.slot_bytes, st) != hipSuccess) return DG_ERR_LAUNCH;

  IscTileArgs g;
  g.a = hist_series(a); g.b = hist_series(b);
  g.xf = hist_xform(s, a->C);
  g.H = H; g.W = W; g.T = a->T; g.nout = l.nout; g.nthr = s->nthr; g.n = l.n; g.tw = l.tw; g.ntiles = l.th * l.tw;
  hist_thr_pad(s->thr, l.nout, s->nthr, g.thr);
  g.slots = slots; g.totals = totals;
  const size_t lds = (size_t)l.njk * 2 * ISC_TILE * sizeof(u64);     // <= ISC_LDS_MAX (static_assert above)
  const unsigned gt = (unsigned)(a->T < ISC_GRID_T ? a->T : ISC_GRID_T);
  const dim3 tgrid((unsigned)g.ntiles, gt), tblock(ISC_THREADS);
  hist_dispatch<false>(a->dtype, hist_mode(a), [&](auto t, auto m) {
    tiles_of<decltype(t), decltype(m)::value>(b, g, tgrid, tblock, lds, st);
  });

  if (l.n > ISC_TILE_LOG) {
    IscPyrArgs pg;
    pg.totals = totals; pg.slots = slots; pg.T = a->T; pg.njk = l.njk; pg.n = l.n; pg.th = l.th; pg.tw = l.tw;
    hipLaunchKernelGGL(iscale_pyramid_kernel, dim3((unsigned)l.njk, gt), dim3(ISC_PYR_THREADS), 0, st, pg);
  }

  const int cnt = l.njk * (l.n + 1) * 3;
  hipLaunchKernelGGL(iscale_finish_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (const u64*)slots, a->T, cnt,
                     reinterpret_cast<u64*>(sums), reinterpret_cast<u64*>(per_field));
  return dg_check_launch();
}
