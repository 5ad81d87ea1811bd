// Joint histograms (include/downgan_hip.h "Joint histograms"): 2-D tables over one or two series of fields read through the EOF
// descriptor (NCHW, [n, H, W, c], padded NHWC; fp32 / bf16), any T and P.
//   joint_kernel<TA, TB, MODE>   one launch per GROUP of consecutive pairs whose uint32 tables together fit the LDS budget of a
//                                workgroup.  Grid-stride over the items (t, pixel group) as hist_kernel: the values of both series,
//                                affine, speed and direction once per pixel, then per pair of the group the two axis indices and one
//                                ds_add_u32 on the cell.  After the loop the non-zero cells are added to counts with 64-bit integer
//                                atomics (the group's LDS layout is its slice of counts: tables in pair order, row-major).
// MODE as hist_kernel (hist_common.h): HIST_NCHW4 / HIST_PIX16 when both series have that mode and one dtype, else HIST_ANY for
// both.  A series no axis of the group reads is not loaded.  Nothing is summed in floating point and no float atomics are used:
// integer counts do not depend on arrival order, so two calls are bit-identical.
#include <float.h>
#include <math.h>

#include "dg_internal.h"
#include "hist_common.h"

namespace {

#ifndef DG_JOINT_LDS_CELLS
#define DG_JOINT_LDS_CELLS 16384                        // uint32 cells per workgroup: 64 KiB, two workgroups per CU
#endif
constexpr int JOINT_LDS_CELLS = DG_JOINT_LDS_CELLS;
constexpr int JOINT_THREADS_MAX = 1024;
constexpr int JOINT_CUS = 256;                          // the grid is the resident workgroups: each flushes its tables once
constexpr long long JOINT_WG_ITEMS_MAX = 1LL << 28;     // items per workgroup per launch: <= 2^30 (+ 4096) values, no uint32 wrap
constexpr int MAXC = DG_EOF_MAX_C, MAXP = DG_HIST2D_MAX_PAIRS, MAXK = DG_HIST2D_MAX_SECTORS / 4;
static_assert(JOINT_LDS_CELLS >= DG_HIST2D_MAX_CELLS && JOINT_LDS_CELLS * 4 <= 160 * 1024 - 1024, "LDS budget");

struct JointAxis {
  int src, chan, nbins;
  float lo, inv_w;
};

struct JointArgs {
  HistSeries s[2];
  int npairs, cells, K;                                 // pairs and cells of this group
  int use[2], need_speed[2], need_dir[2];               // per series: read by an axis of the group / its speed / its direction
  long long t0, items;                                  // fields t0 .. of this launch; items = fields * items per field
  int ipf;
  float calm, tan_k[MAXK];
  HistXform xf;
  JointAxis ax[MAXP][2];
  int off[MAXP];                                        // first cell of the pair's table inside the group
  unsigned long long* counts;                           // the group's slice of counts
};

// the index of one point on one axis (wave-uniform axis): the value is picked by selects, no register array is indexed
__device__ __forceinline__ int joint_axis_bin(const JointAxis& ax, int C, const float (&y)[2][MAXC], const float (&sp)[2],
                                              const int (&dir)[2]) {
  const bool b = ax.src != 0;
  if (ax.chan == C + 1) return b ? dir[1] : dir[0];
  float val = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) val = ax.chan == c ? (b ? y[1][c] : y[0][c]) : val;
  val = ax.chan == C ? (b ? sp[1] : sp[0]) : val;       // after the components: chan = C < MAXC also names a register of y
  return hist_bin(val, ax.lo, ax.inv_w, ax.nbins);
}

template <typename TA, typename TB, int MODE>
__global__ __launch_bounds__(JOINT_THREADS_MAX) void joint_kernel(JointArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned int joint_lds[];   // the group's tables
  for (int i = threadIdx.x; i < a.cells; i += blockDim.x) joint_lds[i] = 0u;
  __syncthreads();
  constexpr int NPX = MODE == HIST_NCHW4 ? 4 : 1;
  // item g = (field t0 + t, item i of the field); the stride is split once so that the loop does no 64-bit division
  const long long stride = (long long)gridDim.x * blockDim.x, g0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long dt = stride / a.ipf, di = stride % a.ipf;
  long long t = a.t0 + g0 / a.ipf, i = g0 % a.ipf;
  for (long long g = g0; g < a.items; g += stride) {
    float va[4][MAXC], vb[4][MAXC];
#pragma unroll
    for (int k = 0; k < NPX; ++k)
#pragma unroll
      for (int c = 0; c < MAXC; ++c) va[k][c] = vb[k][c] = 0.f;
    if (a.use[0]) hist_load_item<TA, MODE>(a.s[0], a.xf.C, t, i, va);
    if (a.use[1]) hist_load_item<TB, MODE>(a.s[1], a.xf.C, t, i, vb);
    t += dt;
    i += di;
    if (i >= a.ipf) { i -= a.ipf; ++t; }
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      float y[2][MAXC], sp[2] = {0.f, 0.f};
      int dir[2] = {0, 0};
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        float yu = 0.f, yv = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          y[r][c] = c < a.xf.C ? hist_affine(r ? vb[k][c] : va[k][c], a.xf.scale[c], a.xf.offset[c]) : 0.f;
          yu = c == a.xf.su ? y[r][c] : yu;
          yv = c == a.xf.sv ? y[r][c] : yv;
        }
        if (a.need_speed[r]) sp[r] = hist_speed(yu, yv);
        if (a.need_dir[r]) dir[r] = hist_dir(yu, yv, sp[r], a.calm, a.K, a.tan_k);
      }
      for (int p = 0; p < a.npairs; ++p) {
        const int bx = joint_axis_bin(a.ax[p][0], a.xf.C, y, sp, dir), by = joint_axis_bin(a.ax[p][1], a.xf.C, y, sp, dir);
        atomicAdd(&joint_lds[a.off[p] + bx * (a.ax[p][1].nbins + 3) + by], 1u);
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < a.cells; c += blockDim.x) {
    const unsigned n = joint_lds[c];
    if (n) atomicAdd(a.counts + c, (unsigned long long)n);
  }
}

long long cells_of(const dg_hist2d_spec* s, int p) { return (long long)(s->ax[p][0].nbins + 3) * (s->ax[p][1].nbins + 3); }

bool spec_ok(const dg_hist2d_spec* s, int C) {
  if (!s || s->npairs < 1 || s->npairs > MAXP || !hist_xform_ok(s, C)) return false;
  const bool speed = s->speed_u >= 0;
  if (!hist_finite(s->calm) || s->calm < 0.f) return false;
  if (s->nsec != 0 && (s->nsec < 4 || s->nsec > DG_HIST2D_MAX_SECTORS || s->nsec % 4 != 0)) return false;
  for (int p = 0; p < s->npairs; ++p) {
    for (int e = 0; e < 2; ++e) {
      const dg_hist2d_axis& ax = s->ax[p][e];
      if ((ax.src != 0 && ax.src != 1) || ax.chan < 0 || ax.chan > C + 1 || ax.nbins < 1 || ax.nbins > DG_HIST2D_MAX_CELLS) return false;
      if (ax.chan >= C && !speed) return false;
      if (ax.chan == C + 1) {
        if (s->nsec == 0 || ax.nbins != s->nsec) return false;
        for (int k = 1; k < s->nsec / 4; ++k)
          if (!(s->tan_k[k] > 0.f && s->tan_k[k] <= FLT_MAX)) return false;
      } else if (!hist_finite(ax.lo) || !(ax.inv_w > 0.f && ax.inv_w <= FLT_MAX)) {
        return false;
      }
    }
    if (cells_of(s, p) > DG_HIST2D_MAX_CELLS) return false;
  }
  return true;
}

bool uses_b(const dg_hist2d_spec* s) {
  for (int p = 0; p < s->npairs; ++p)
    if (s->ax[p][0].src == 1 || s->ax[p][1].src == 1) return true;
  return false;
}

bool call_ok(const dg_eof_fields* a, const dg_eof_fields* b, const dg_hist2d_spec* s) {
  if (!hist_fields_ok(a) || !spec_ok(s, a->C)) return false;
  if (b && (!hist_fields_ok(b) || b->T != a->T || b->C != a->C || b->P != a->P)) return false;
  return b || !uses_b(s);
}

bool dtype_ok(const dg_eof_fields* x) { return x->dtype == DG_F32 || x->dtype == DG_BF16; }

template <typename TA, typename TB, int MODE>
int launch(const JointArgs& a, int grid, int threads, hipStream_t st) {
  DG_SET_MAX_LDS_ONCE((joint_kernel<TA, TB, MODE>), (int)(JOINT_LDS_CELLS * sizeof(unsigned)));
  hipLaunchKernelGGL((joint_kernel<TA, TB, MODE>), dim3(grid), dim3(threads), (size_t)a.cells * sizeof(unsigned), st, a);
  return DG_OK;
}

template <int MODE>
int launch_same(bool bf16, const JointArgs& a, int grid, int threads, hipStream_t st) {
  return bf16 ? launch<bf16_t, bf16_t, MODE>(a, grid, threads, st) : launch<float, float, MODE>(a, grid, threads, st);
}

int launch_any(bool a_bf16, bool b_bf16, const JointArgs& a, int grid, int threads, hipStream_t st) {
  if (a_bf16) return b_bf16 ? launch<bf16_t, bf16_t, HIST_ANY>(a, grid, threads, st) : launch<bf16_t, float, HIST_ANY>(a, grid, threads, st);
  return b_bf16 ? launch<float, bf16_t, HIST_ANY>(a, grid, threads, st) : launch<float, float, HIST_ANY>(a, grid, threads, st);
}

}  // namespace

extern "C" size_t dg_hist2d_ws_bytes(const dg_eof_fields* a, const dg_eof_fields* b, const dg_hist2d_spec* s) {
  return call_ok(a, b, s) ? 256 : 0;                    // no workspace is needed: 0 stays "invalid"
}

extern "C" int dg_hist2d_host_bins(const dg_hist2d_spec* s, const float* xa, const float* xb, int C, int64_t n, int32_t* bins) {
  if (!spec_ok(s, C) || n < 0 || (n > 0 && (!xa || !bins)) || (n > 0 && !xb && uses_b(s))) return DG_ERR_BAD_SHAPE;
  const int K = s->nsec / 4, nout = hist_nout(s, C);
  for (int64_t i = 0; i < n; ++i) {
    float y[2][HIST_MAXO] = {};                           // every output value of the point, once per series
    for (int r = 0; r < 2; ++r)
      if (const float* x = r ? xb : xa)                   // an axis on xb without xb: refused above
        for (int j = 0; j < nout; ++j) y[r][j] = hist_host_value(s, x, C, (size_t)n, (size_t)i, j);
    for (int p = 0; p < s->npairs; ++p) {
      for (int e = 0; e < 2; ++e) {
        const dg_hist2d_axis& ax = s->ax[p][e];
        const float* yr = y[ax.src];
        bins[((int64_t)p * 2 + e) * n + i] = ax.chan == C + 1 ? hist_dir(yr[s->speed_u], yr[s->speed_v], yr[C], s->calm, K, s->tan_k)
                                                              : hist_bin(yr[ax.chan], ax.lo, ax.inv_w, ax.nbins);
      }
    }
  }
  return DG_OK;
}

extern "C" int dg_hist2d(const dg_eof_fields* a, const dg_eof_fields* b, const dg_hist2d_spec* s, void* ws, int64_t* counts,
                         void* stream) {
  if (!call_ok(a, b, s) || !ws || !counts) return DG_ERR_BAD_SHAPE;
  if (!dtype_ok(a) || (b && !dtype_ok(b))) return DG_ERR_BAD_DTYPE;
  const bool two = b != nullptr && uses_b(s);
  const dg_eof_fields* fb = two ? b : a;
  // fast paths: both series in one mode and dtype; anything else reads element by element
  int mode = hist_mode(a);
  if (two && (hist_mode(b) != mode || b->dtype != a->dtype)) mode = HIST_ANY;
  JointArgs g;
  g.s[0] = hist_series(a);
  g.s[1] = hist_series(fb);
  g.xf = hist_xform(s, a->C);
  g.K = s->nsec / 4;
  g.calm = s->calm;
  for (int k = 0; k < MAXK; ++k) g.tan_k[k] = k >= 1 && k < g.K ? s->tan_k[k] : 0.f;
  g.ipf = mode == HIST_NCHW4 ? a->P / 4 : a->P;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  long long done = 0;                                   // cells of the groups before this one
  for (int p0 = 0; p0 < s->npairs;) {
    // the group: consecutive pairs while their tables fit the budget
    int np = 0;
    long long cells = 0;
    for (int r = 0; r < 2; ++r) g.use[r] = g.need_speed[r] = g.need_dir[r] = 0;
    while (p0 + np < s->npairs && cells + cells_of(s, p0 + np) <= JOINT_LDS_CELLS) {
      g.off[np] = (int)cells;
      for (int e = 0; e < 2; ++e) {
        const dg_hist2d_axis& ax = s->ax[p0 + np][e];
        g.ax[np][e] = JointAxis{ax.src, ax.chan, ax.nbins, ax.lo, ax.inv_w};
        g.use[ax.src] = 1;
        if (ax.chan >= a->C) g.need_speed[ax.src] = 1;  // the direction rule reads the speed too
        if (ax.chan == a->C + 1) g.need_dir[ax.src] = 1;
      }
      cells += cells_of(s, p0 + np);
      ++np;
    }
    for (int q = np; q < MAXP; ++q) {
      g.off[q] = 0;
      g.ax[q][0] = g.ax[q][1] = JointAxis{0, 0, 1, 0.f, 1.f};
    }
    g.npairs = np; g.cells = (int)cells;
    g.counts = reinterpret_cast<unsigned long long*>(counts) + done;
    // two workgroups of 512 threads per CU while two tables fit its LDS, else one of 1024: 16 waves per CU either way
    const bool big = cells * sizeof(unsigned) > 72 * 1024;
    const int threads = big ? 1024 : 512, grid_max = big ? JOINT_CUS : 2 * JOINT_CUS;
    // fields per launch: at most JOINT_WG_ITEMS_MAX items per workgroup, so no uint32 cell can wrap
    const long long tmax = (long long)grid_max * JOINT_WG_ITEMS_MAX / g.ipf;
    for (long long t0 = 0; t0 < a->T; t0 += tmax) {
      const long long nt = a->T - t0 < tmax ? a->T - t0 : tmax;
      g.t0 = t0;
      g.items = nt * g.ipf;
      const long long want = (g.items + threads - 1) / threads;
      const int grid = (int)(want < 1 ? 1 : want > grid_max ? grid_max : want);
      const bool abf = a->dtype == DG_BF16, bbf = fb->dtype == DG_BF16;
      const int rc = mode == HIST_NCHW4 ? launch_same<HIST_NCHW4>(abf, g, grid, threads, st)
                   : mode == HIST_PIX16 ? launch_same<HIST_PIX16>(abf, g, grid, threads, st) : launch_any(abf, bbf, g, grid, threads, st);
      if (rc != DG_OK) return rc;
    }
    done += cells;
    p0 += np;
  }
  return dg_check_launch();
}
