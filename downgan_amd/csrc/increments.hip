// Increment histograms (include/downgan_hip.h "Increment histograms"): the distributions of the spatial increments
// d = y(x + r) - y(x) of one or two series of H x W fields read through the EOF descriptor (NCHW, [n, H, W, c], padded NHWC;
// fp32 / bf16), per output channel, direction (0 along w, 1 along h) and lag.
//   incr_kernel<T, MODE>   one launch per (series, direction, GROUP of output channels whose uint32 tables fit the table part of
//                          the LDS).  A workgroup walks tiles (field, row block, column block).  Per output channel of the group
//                          it stages the transformed values y of the tile -- affine and speed once per staged pixel -- with a halo
//                          of the largest lag of the launch's direction in LDS, then every thread takes anchors of the tile: y0
//                          once, and per lag the partner from LDS, hist_diff, hist_bin, one ds_add_u32 on the cell and the six
//                          fp64 terms into registers.  The registers are reduced per (tile, channel): butterfly over the wave,
//                          then the waves in order into the workgroup's fp64 sums in LDS.  After the last tile the non-zero cells
//                          go to counts / finite with 64-bit integer atomics and the fp64 sums to the workgroup's workspace slot.
//                          direction 0: tiles of AH rows x (512 + halo) columns; direction 1: strips of (AH + halo) rows x 64
//                          columns (global loads stay 128 - 256 B per row); AH from the tile part of the LDS.
//   incr_finish_kernel     one workgroup per (channel of the group, lag): the slots summed in workgroup order (fixed), += moments
// MODE as hist_kernel (hist_common.h): HIST_NCHW4 only when W % 4 == 0 (the rows of an odd W are not 16-byte aligned even when
// P % 4 == 0: those fields take the element path), HIST_PIX16, HIST_ANY.
// Integer counts do not depend on arrival order and nothing else is summed by atomics, so two calls are bit-identical.
// Build macros (A/B only, Makefile targets incr_naive / incr_sub4; tools/incr_bench.py --lib):
//   DG_INCR_NAIVE          no tile: both operands of every increment are read from global memory and transformed again
//   DG_INCR_SUBTABLES=S    S copies of the tables per workgroup, wave w adds to copy w % S (S a power of two)
#include <float.h>
#include <math.h>

#include <vector>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

#ifndef DG_INCR_SUBTABLES
#define DG_INCR_SUBTABLES 1
#endif
constexpr int SUB = DG_INCR_SUBTABLES;
constexpr int INCR_THREADS = 512, INCR_WAVES = INCR_THREADS / 64;   // 8 waves: the 48 fp64 sums of a thread need > 128 VGPRs
constexpr int INCR_CUS = 256;                           // the grid is the resident workgroups (one per CU): each flushes once
constexpr int INCR_TABLE_CELLS = 12288;                 // uint32 cells of a group's tables: 48 KiB
constexpr int INCR_TILE_FLOATS = 24576;                 // the staged tile of one output channel: 96 KiB
constexpr int INCR_AW0 = 512, INCR_AW1 = 64;            // anchor columns of a tile, direction 0 / 1
constexpr long long INCR_WG_TILES_MAX = 131072;         // tiles per workgroup per launch: (2^17 + 1) * 24576 < 2^32, no wrap
constexpr int MAXO = DG_HIST_MAX_OUT, MAXL = DG_INCR_MAX_LAGS;
static_assert((SUB & (SUB - 1)) == 0 && SUB >= 1 && SUB <= INCR_WAVES, "sub-tables");
static_assert(MAXL * (DG_INCR_MAX_BINS + 4) <= INCR_TABLE_CELLS, "one output channel must fit the table budget");
static_assert((INCR_TABLE_CELLS + INCR_TILE_FLOATS) * 4 + 8192 <= 160 * 1024, "LDS budget");
static_assert(INCR_TILE_FLOATS / ((INCR_AW0 + DG_INCR_MAX_LAG + 3) / 4 * 4) >= 1 && INCR_TILE_FLOATS / INCR_AW1 > DG_INCR_MAX_LAG, "tile");
static_assert((INCR_WG_TILES_MAX + 1) * INCR_TILE_FLOATS < (1LL << 32), "no uint32 wrap");

struct IncrArgs {
  HistSeries x;
  int C, H, W, su, sv;                                  // C, su, sv, scale, offset: HistXform's members, not embedded (run_series)
  int nlag, nbins, dir, sub;                            // sub: copies of the tables (SUB, fewer when they would not fit)
  int R, CW, AH, AW, tiles_h, tiles_w;                  // tile rows / columns staged, anchor rows / columns, tiles per field
  long long t0, ntiles;                                 // fields t0 .. of this launch; ntiles = fields * tiles per field
  int jn, chan[MAXO];                                   // the output channels of this group
  int lag[MAXL];
  float scale[HIST_MAXC], offset[HIST_MAXC];
  float lo[MAXO][MAXL], inv_w[MAXO][MAXL];              // [channel of the group][lag]
  unsigned long long* counts;                           // the series' [nout][2][nlag][nbins + 3]
  unsigned long long* finite;                           // the series' [nout][2][nlag]
  double* part;                                         // [grid][MAXO][MAXL][6]
};

// the six terms of one increment (shared with the host reference)
struct IncrTerms { double v[6]; };
__host__ __device__ inline IncrTerms incr_terms(float d) {
#pragma clang fp contract(off)
  const double u = (double)d, u2 = u * u, u3 = u2 * u, u4 = u2 * u2;
  return IncrTerms{{u, __builtin_fabs(u), u2, u3, __builtin_fabs(u3), u4}};
}

// output channel j of pixel p of one field, element by element
template <typename T>
__device__ __forceinline__ float incr_value(const IncrArgs& a, const T* f, int j, long long p) {
  const T* q = f + p * a.x.ld_p;
  if (j < a.C) return hist_affine(ld_elem(q + j * a.x.ld_c), a.scale[j], a.offset[j]);
  return hist_speed(hist_affine(ld_elem(q + a.su * a.x.ld_c), a.scale[a.su], a.offset[a.su]),
                    hist_affine(ld_elem(q + a.sv * a.x.ld_c), a.scale[a.sv], a.offset[a.sv]));
}

template <typename T, int MODE>
__global__ __launch_bounds__(INCR_THREADS) void incr_kernel(IncrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned int incr_lds[];    // [sub][jn][nlag][nbins + 4], then the tile
  __shared__ double red[INCR_WAVES][MAXL][6];
  __shared__ double wg_sum[MAXO][MAXL][6];
  const int nb4 = a.nbins + 4;                          // a table and, as its last cell, the number of finite increments
  const int gcells = a.jn * a.nlag * nb4;
  float* tile = reinterpret_cast<float*>(incr_lds + ((a.sub * gcells + 3) & ~3));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < a.sub * gcells; i += INCR_THREADS) incr_lds[i] = 0u;
  for (int i = tid; i < MAXO * MAXL * 6; i += INCR_THREADS) (&wg_sum[0][0][0])[i] = 0.0;
  unsigned int* tab = incr_lds + (wave & (a.sub - 1)) * gcells;
  const int tpf = a.tiles_h * a.tiles_w;
  const int ext = a.dir ? a.H : a.W;
  int poff[MAXL];                                       // the partner's distance in the tile
#pragma unroll
  for (int l = 0; l < MAXL; ++l) poff[l] = l < a.nlag ? (a.dir ? a.lag[l] * a.CW : a.lag[l]) : 0;
  __syncthreads();
  for (long long id = blockIdx.x; id < a.ntiles; id += gridDim.x) {
    const long long t = a.t0 + id / tpf;
    const int ti = (int)(id % tpf), th = ti / a.tiles_w, tw = ti - th * a.tiles_w;
    const int h0 = th * a.AH, w0 = tw * a.AW;
    const int re = min(a.R, a.H - h0), ce = min(a.CW, a.W - w0);         // rows / columns staged
    const int ah = min(a.AH, a.H - h0), aw = min(a.AW, a.W - w0);        // anchor rows / columns
    const T* f = reinterpret_cast<const T*>(a.x.base) + t * a.x.ld_t;
    for (int jj = 0; jj < a.jn; ++jj) {
      const int j = a.chan[jj];
#ifndef DG_INCR_NAIVE
      const bool spd = j >= a.C;
      const int c0 = spd ? a.su : j, c1 = spd ? a.sv : j;
      const float sc0 = a.scale[c0], of0 = a.offset[c0], sc1 = a.scale[c1], of1 = a.offset[c1];
      if (MODE == HIST_NCHW4) {                         // W % 4 == 0, w0 % 4 == 0, ce % 4 == 0: every load is aligned
        const int c4n = ce >> 2;
        for (int i = tid; i < re * c4n; i += INCR_THREADS) {
          const int r = i / c4n, q = i - r * c4n;
          const T* p = f + (long long)(h0 + r) * a.W + w0 + 4 * q;
          float v0[4], v1[4];
          ld4(p + c0 * a.x.ld_c, v0);
          if (spd) ld4(p + c1 * a.x.ld_c, v1);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float y = hist_affine(v0[k], sc0, of0);
            tile[r * a.CW + 4 * q + k] = spd ? hist_speed(y, hist_affine(v1[k], sc1, of1)) : y;
          }
        }
      } else if (MODE == HIST_PIX16) {
        for (int i = tid; i < re * ce; i += INCR_THREADS) {
          const int r = i / ce, c = i - r * ce;
          const uint4 px = *reinterpret_cast<const uint4*>(f + ((long long)(h0 + r) * a.W + w0 + c) * a.x.ld_p);
          const float y = hist_affine(hist_pick16_sel<T>(px, c0), sc0, of0);
          tile[r * a.CW + c] = spd ? hist_speed(y, hist_affine(hist_pick16_sel<T>(px, c1), sc1, of1)) : y;
        }
      } else {
        for (int i = tid; i < re * ce; i += INCR_THREADS) {
          const int r = i / ce, c = i - r * ce;
          tile[r * a.CW + c] = incr_value<T>(a, f, j, (long long)(h0 + r) * a.W + w0 + c);
        }
      }
      __syncthreads();
#endif
      double m[MAXL][6];
      unsigned nf[MAXL];
#pragma unroll
      for (int l = 0; l < MAXL; ++l) {
        nf[l] = 0u;
#pragma unroll
        for (int k = 0; k < 6; ++k) m[l][k] = 0.0;
      }
      for (int i = tid; i < ah * aw; i += INCR_THREADS) {
        const int r = i / aw, c = i - r * aw;
        const int pos = a.dir ? h0 + r : w0 + c;
#ifndef DG_INCR_NAIVE
        const float* y = tile + r * a.CW + c;
        const float y0 = y[0];
#else
        const long long p0 = (long long)(h0 + r) * a.W + w0 + c;
        const float y0 = incr_value<T>(a, f, j, p0);
#endif
#pragma unroll
        for (int l = 0; l < MAXL; ++l) {
          if (l < a.nlag && pos + a.lag[l] < ext) {     // the partner lies in the grid, hence in the tile
#ifndef DG_INCR_NAIVE
            const float d = hist_diff(y[poff[l]], y0);
#else
            const float d = hist_diff(incr_value<T>(a, f, j, p0 + (a.dir ? (long long)a.lag[l] * a.W : a.lag[l])), y0);
#endif
            atomicAdd(&tab[(jj * a.nlag + l) * nb4 + hist_bin(d, a.lo[jj][l], a.inv_w[jj][l], a.nbins)], 1u);
            const bool fin = hist_finite(d);
            const IncrTerms e = incr_terms(fin ? d : 0.f);
            nf[l] += fin ? 1u : 0u;
#pragma unroll
            for (int k = 0; k < 6; ++k) m[l][k] += e.v[k];
          }
        }
      }
      // butterfly over the wave (the same order in every lane), then the waves in order
#pragma unroll
      for (int l = 0; l < MAXL; ++l) {
        if (l < a.nlag) {
          for (int s = 32; s >= 1; s >>= 1) {
            nf[l] += __shfl_xor(nf[l], s, 64);
#pragma unroll
            for (int k = 0; k < 6; ++k) m[l][k] += hist_shfl_xor_f64(m[l][k], s);
          }
          if (lane == 0) {
            if (nf[l]) atomicAdd(&tab[(jj * a.nlag + l) * nb4 + a.nbins + 3], nf[l]);
#pragma unroll
            for (int k = 0; k < 6; ++k) red[wave][l][k] = m[l][k];
          }
        }
      }
      __syncthreads();                                  // red is complete, and nobody reads the tile any more
      if (tid < a.nlag * 6) {
        const int l = tid / 6, k = tid - l * 6;
        double s = wg_sum[jj][l][k];
        for (int w = 0; w < INCR_WAVES; ++w) s += red[w][l][k];
        wg_sum[jj][l][k] = s;
      }
#ifdef DG_INCR_NAIVE
      __syncthreads();                                  // (the tiled kernel has the barrier after the next fill in between)
#endif
    }
  }
  __syncthreads();
  const int nb3 = a.nbins + 3;
  for (int i = tid; i < gcells; i += INCR_THREADS) {
    unsigned long long n = 0;
    for (int s = 0; s < a.sub; ++s) n += incr_lds[s * gcells + i];
    if (n) {
      const int q = i / nb4, cell = i - q * nb4, jj = q / a.nlag, l = q - jj * a.nlag;
      const long long row = ((long long)a.chan[jj] * 2 + a.dir) * a.nlag + l;
      atomicAdd(cell < nb3 ? a.counts + row * nb3 + cell : a.finite + row, n);
    }
  }
  for (int i = tid; i < MAXO * MAXL * 6; i += INCR_THREADS) a.part[(long long)blockIdx.x * (MAXO * MAXL * 6) + i] = (&wg_sum[0][0][0])[i];
}

// one workgroup per (channel of the group, lag): thread i sums the slots i, i + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void incr_finish_kernel(const double* part, int grid, IncrArgs a, double* moments) {
  __shared__ double sm[256][6];
  const int jj = blockIdx.x / a.nlag, l = blockIdx.x - jj * a.nlag;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int g = threadIdx.x; g < grid; g += 256) {
    const double* p = part + (long long)g * (MAXO * MAXL * 6) + (jj * MAXL + l) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += p[k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) sm[threadIdx.x][k] = s[k];
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (threadIdx.x < h)
#pragma unroll
      for (int k = 0; k < 6; ++k) sm[threadIdx.x][k] += sm[threadIdx.x + h][k];
    __syncthreads();
  }
  if (threadIdx.x < 6) moments[(((long long)a.chan[jj] * 2 + a.dir) * a.nlag + l) * 6 + threadIdx.x] += sm[0][threadIdx.x];
}

bool spec_ok(const dg_incr_spec* s, int C) {
  if (!s || s->nlag < 1 || s->nlag > MAXL || s->nbins < 1 || s->nbins > DG_INCR_MAX_BINS || !hist_xform_ok(s, C)) return false;
  for (int l = 0; l < s->nlag; ++l)
    if (s->lag[l] < 1 || s->lag[l] > DG_INCR_MAX_LAG || (l > 0 && s->lag[l] <= s->lag[l - 1])) return false;
  for (int j = 0; j < hist_nout(s, C); ++j)
    for (int l = 0; l < s->nlag; ++l)
      if (!hist_finite(s->lo[j][l]) || !(s->inv_w[j][l] > 0.f && s->inv_w[j][l] <= FLT_MAX)) return false;
  return true;
}

bool grid_ok(int H, int W) { return H >= 1 && H <= DG_INCR_MAX_SIDE && W >= 1 && W <= DG_INCR_MAX_SIDE; }

bool call_ok(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_incr_spec* s) {
  if (!hist_fields_ok(a) || !grid_ok(H, W) || (long long)H * W != a->P || !spec_ok(s, a->C)) return false;
  return !b || (hist_fields_ok(b) && b->T == a->T && b->C == a->C && b->P == a->P);
}

bool dtype_ok(const dg_eof_fields* x) { return x->dtype == DG_F32 || x->dtype == DG_BF16; }

template <typename T, int MODE>
int launch(const IncrArgs& a, int grid, size_t lds, hipStream_t st) {
  DG_SET_MAX_LDS_ONCE((incr_kernel<T, MODE>), (int)((INCR_TABLE_CELLS + INCR_TILE_FLOATS) * sizeof(unsigned)));
  hipLaunchKernelGGL((incr_kernel<T, MODE>), dim3(grid), dim3(INCR_THREADS), lds, st, a);
  return DG_OK;
}

constexpr size_t INCR_WS_BYTES = (size_t)INCR_CUS * MAXO * MAXL * 6 * sizeof(double);

// one series: both directions, every group of output channels
int run_series(const dg_eof_fields* x, int H, int W, const dg_incr_spec* s, void* ws, int64_t* counts, int64_t* finite,
               double* moments, hipStream_t st) {
  const int C = x->C, nout = hist_nout(s, C), nb4 = s->nbins + 4;
  int mode = hist_mode(x);
  if (mode == HIST_NCHW4 && W % 4 != 0) mode = HIST_ANY;                 // rows of such a W are not 16-byte aligned
  IncrArgs g;
  g.x = hist_series(x);
  // incr_kernel runs at 106 SGPRs and reads its arguments again inside its loops.  With a HistXform embedded in front of H / W
  // it took 0.5 - 0.7 % longer on Gaussian fields at the same registers (profiles/field_reader_refactor.json), so the argument
  // layout stays as it was measured and the padded transform is copied in member by member.
  const HistXform xf = hist_xform(s, C);
  g.C = xf.C; g.H = H; g.W = W; g.su = xf.su; g.sv = xf.sv;
  for (int c = 0; c < HIST_MAXC; ++c) { g.scale[c] = xf.scale[c]; g.offset[c] = xf.offset[c]; }
  g.nbins = s->nbins;
  g.counts = reinterpret_cast<unsigned long long*>(counts);
  g.finite = reinterpret_cast<unsigned long long*>(finite);
  g.part = reinterpret_cast<double*>(ws);
  int sub = SUB;
  while (sub > 1 && sub * s->nlag * nb4 > INCR_TABLE_CELLS) sub >>= 1;
  g.sub = sub;
  const int jmax = INCR_TABLE_CELLS / (sub * s->nlag * nb4);             // output channels per group (>= 1)
  for (int dir = 0; dir < 2; ++dir) {
    const int ext = dir ? H : W;
    int nl = 0;                                                           // lags below the extent: the others contribute nothing
    while (nl < s->nlag && s->lag[nl] < ext) ++nl;
    if (nl == 0) continue;
    const int L = s->lag[nl - 1];
    g.dir = dir;
    // the launch keeps the spec's nlag as the row stride of its tables and of the outputs; lags >= ext never pass the bounds test
    g.nlag = s->nlag;
    for (int l = 0; l < MAXL; ++l) g.lag[l] = l < s->nlag ? s->lag[l] : 0;
    if (dir == 0) {
      g.AW = W < INCR_AW0 ? W : INCR_AW0;
      const int span = g.AW + L < W ? g.AW + L : W;
      g.CW = (span + 3) / 4 * 4;
      const int rows = INCR_TILE_FLOATS / g.CW;
      g.AH = g.R = H < rows ? H : rows;
    } else {
      g.AW = W < INCR_AW1 ? W : INCR_AW1;
      g.CW = (g.AW + 3) / 4 * 4;
      const int rows = INCR_TILE_FLOATS / g.CW;                           // >= 384 > L
      g.AH = H < rows - L ? H : rows - L;
      g.R = g.AH + L;
    }
    g.tiles_h = (H + g.AH - 1) / g.AH;
    g.tiles_w = (W + g.AW - 1) / g.AW;
    const long long tpf = (long long)g.tiles_h * g.tiles_w;
    long long tmax = (long long)INCR_CUS * INCR_WG_TILES_MAX / tpf;       // fields per launch: no uint32 cell can wrap
    if (tmax < 1) tmax = 1;
    for (int j0 = 0; j0 < nout; j0 += jmax) {
      g.jn = nout - j0 < jmax ? nout - j0 : jmax;
      for (int jj = 0; jj < MAXO; ++jj) {
        g.chan[jj] = jj < g.jn ? j0 + jj : 0;
        for (int l = 0; l < MAXL; ++l) {
          const bool on = jj < g.jn && l < s->nlag;
          g.lo[jj][l] = on ? s->lo[j0 + jj][l] : 0.f;
          g.inv_w[jj][l] = on ? s->inv_w[j0 + jj][l] : 1.f;
        }
      }
      const size_t lds = ((size_t)((sub * g.jn * g.nlag * nb4 + 3) & ~3) + (size_t)g.R * g.CW) * sizeof(unsigned);
      for (long long t0 = 0; t0 < x->T; t0 += tmax) {
        const long long nt = x->T - t0 < tmax ? x->T - t0 : tmax;
        g.t0 = t0;
        g.ntiles = nt * tpf;
        const int grid = (int)(g.ntiles < INCR_CUS ? g.ntiles : INCR_CUS);
        const int rc = hist_dispatch(x->dtype, mode, [&](auto t, auto m) { return launch<decltype(t), decltype(m)::value>(g, grid, lds, st); });
        if (rc != DG_OK) return rc;
        hipLaunchKernelGGL(incr_finish_kernel, dim3(g.jn * g.nlag), dim3(256), 0, st, (const double*)g.part, grid, g, moments);
      }
    }
  }
  return DG_OK;
}

}  // namespace

extern "C" size_t dg_incr_ws_bytes(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_incr_spec* s) {
  return call_ok(a, b, H, W, s) ? INCR_WS_BYTES : 0;
}

extern "C" int dg_incr_host(const dg_incr_spec* s, const float* x, int C, int H, int W, int64_t* counts, int64_t* finite,
                            double* moments) {
  if (!spec_ok(s, C) || !grid_ok(H, W) || !x || !counts || !finite || !moments) return DG_ERR_BAD_SHAPE;
  const int nout = hist_nout(s, C), nb3 = s->nbins + 3;
  const size_t P = (size_t)H * W;
  std::vector<float> y((size_t)nout * P);
  for (int j = 0; j < nout; ++j)
    for (size_t p = 0; p < P; ++p) y[j * P + p] = hist_host_value(s, x, C, P, p, j);
  for (int j = 0; j < nout; ++j) {
    const float* yj = y.data() + j * P;
    for (int dir = 0; dir < 2; ++dir) {
      for (int l = 0; l < s->nlag; ++l) {
        const int r = s->lag[l];
        const size_t row = ((size_t)j * 2 + dir) * s->nlag + l;
        const int hn = dir ? H - r : H, wn = dir ? W : W - r;             // anchors; none when the lag reaches the extent
        const size_t step = dir ? (size_t)r * W : (size_t)r;
        for (int h = 0; h < hn; ++h) {
          for (int w = 0; w < wn; ++w) {
            const size_t p = (size_t)h * W + w;
            const float d = hist_diff(yj[p + step], yj[p]);
            counts[row * nb3 + hist_bin(d, s->lo[j][l], s->inv_w[j][l], s->nbins)] += 1;
            if (hist_finite(d)) {
              const IncrTerms e = incr_terms(d);
              finite[row] += 1;
              for (int k = 0; k < 6; ++k) moments[row * 6 + k] += e.v[k];
            }
          }
        }
      }
    }
  }
  return DG_OK;
}

extern "C" int dg_incr(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_incr_spec* s, void* ws,
                       int64_t* counts, int64_t* finite, double* moments, void* stream) {
  if (!call_ok(a, b, H, W, s) || !ws || !counts || !finite || !moments) return DG_ERR_BAD_SHAPE;
  if (!dtype_ok(a) || (b && !dtype_ok(b))) return DG_ERR_BAD_DTYPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long long nout = hist_nout(s, a->C), rows = nout * 2 * s->nlag;
  for (int ser = 0; ser < (b ? 2 : 1); ++ser) {
    const int rc = run_series(ser ? b : a, H, W, s, ws, counts + ser * rows * (s->nbins + 3), finite + ser * rows,
                              moments + ser * rows * 6, st);
    if (rc != DG_OK) return rc;
  }
  return dg_check_launch();
}
