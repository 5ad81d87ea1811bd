// Host memory-safety check of dg_iscale_host (csrc/iscale.hip): the host reference of the intensity-scale sums on small fixed
// inputs with closed-form answers (one aligned block of side 2^m against an empty field, a checkerboard, identical fields, all ones
// against all zeros, a NaN field, a ragged grid against the same pixels on its padded square) on the grids 1 x 1, 1 x W, H x 1,
// ragged ones and W = 2048, compiled with the address and undefined-behaviour sanitizers on the HOST side only and run on the CPU
// (no GPU is touched: the function launches nothing).  Build and run from the repository root:
//   mkdir -p build
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -c downgan_amd/csrc/iscale.hip -o build/iscale_host_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o build/iscale_host_check \
//         tools/iscale_host_check.cpp build/iscale_host_san.o -L$ROCM_PATH/lib -lamdhip64 -Wl,-rpath,$ROCM_PATH/lib
//   ./build/iscale_host_check
// The arrays are allocated at exactly the size the contract states, so a read or write past one is caught.
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#include "../include/downgan_hip.h"

static dg_iscale_spec spec_of(int C, bool speed, int nthr) {
  dg_iscale_spec s{};
  s.speed_u = speed ? 0 : -1;
  s.speed_v = speed ? C - 1 : -1;
  s.nthr = nthr;
  const float thr[DG_ISCALE_MAX_THR] = {0.5f, 2.f, -1.f, 0.f};
  for (int c = 0; c < C; ++c) { s.scale[c] = 1.f; s.offset[c] = 0.f; }
  for (int j = 0; j < C + (speed ? 1 : 0); ++j)
    for (int k = 0; k < nthr; ++k) s.thr[j][k] = thr[k];
  return s;
}

static int64_t pow4(int e) { return (int64_t)1 << (2 * e); }

// one channel, threshold 0.5: sums [n + 1][3] of the pair (a, b), exactly n + 1 levels allocated
static std::vector<int64_t> sums_of(const std::vector<float>& a, const std::vector<float>& b, int H, int W) {
  const dg_iscale_spec s = spec_of(1, false, 1);
  std::vector<int64_t> out((size_t)dg_iscale_levels(H, W) * 3, 0);
  if (dg_iscale_host(&s, a.data(), b.data(), 1, H, W, out.data()) != DG_OK) out.clear();
  return out;
}

static int report(const char* what, int H, int W, int bad) {
  printf("%-28s %4d x %4d: %s\n", what, H, W, bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}

// a block of side 2^m at (y, x) (aligned) against an empty field: E_l = 4^(m + l) for l <= m, 16^m above
static int block(int H, int W, int m, int y, int x) {
  std::vector<float> a((size_t)H * W, 0.f), b((size_t)H * W, 0.f);
  for (int h = y; h < y + (1 << m); ++h)
    for (int w = x; w < x + (1 << m); ++w) a[(size_t)h * W + w] = 1.f;
  const std::vector<int64_t> s = sums_of(a, b, H, W);
  const int n = dg_iscale_levels(H, W) - 1;
  int bad = s.empty();
  for (int l = 0; !bad && l <= n; ++l) {
    const int64_t want = l <= m ? pow4(m + l) : pow4(2 * m);
    bad += s[l * 3] != want || s[l * 3 + 1] != want || s[l * 3 + 2] != 0;
  }
  return report("aligned block", H, W, bad);
}

// a checkerboard on a dyadic square against an empty field: E_0 = P / 2, E_l = P 4^l / 4
static int checkerboard(int N) {
  std::vector<float> a((size_t)N * N), b((size_t)N * N, 0.f);
  for (int h = 0; h < N; ++h)
    for (int w = 0; w < N; ++w) a[(size_t)h * N + w] = (h + w) % 2 ? 0.f : 1.f;
  const std::vector<int64_t> s = sums_of(a, b, N, N);
  const int n = dg_iscale_levels(N, N) - 1;
  const int64_t P = (int64_t)N * N;
  int bad = s.empty();
  for (int l = 0; !bad && l <= n; ++l) {
    const int64_t want = l == 0 ? P / 2 : P * pow4(l) / 4;
    bad += s[l * 3] != want || s[l * 3 + 1] != want || s[l * 3 + 2] != 0;
  }
  return report("checkerboard", N, N, bad);
}

// every pixel set (fill 1) or NaN against zeros, any grid: E_l = sum over the blocks of (pixels of the block inside the grid)^2
static int constant(int H, int W, float fill) {
  std::vector<float> a((size_t)H * W, fill), b((size_t)H * W, 0.f);
  const std::vector<int64_t> s = sums_of(a, b, H, W);
  const int n = dg_iscale_levels(H, W) - 1;
  int bad = s.empty();
  for (int l = 0; !bad && l <= n; ++l) {
    const int64_t bs = (int64_t)1 << l;
    // full blocks and one partial block per direction: rows = (H / bs) blocks of bs and one of H % bs
    const int64_t rows2 = (H / bs) * bs * bs + (H % bs) * (H % bs), cols2 = (W / bs) * bs * bs + (W % bs) * (W % bs);
    const int64_t want = fill == fill ? rows2 * cols2 : 0;             // NaN exceeds nothing
    bad += s[l * 3] != want || s[l * 3 + 1] != want || s[l * 3 + 2] != 0;
  }
  bad += dg_iscale_bound(H, W) != pow4(2 * n);
  return report(fill == fill ? "all ones against zeros" : "NaN against zeros", H, W, bad);
}

// pseudo-random pair: identical fields give D = 0 and A = B; a ragged grid equals the same pixels stored on its padded square;
// every output of the largest spec (8 channels + speed, 4 thresholds) is written and nothing beyond
static int random_pair(int H, int W) {
  const int n = dg_iscale_levels(H, W) - 1, S = 1 << n;
  std::vector<float> a((size_t)H * W), b((size_t)H * W), pa((size_t)S * S, 0.f), pb((size_t)S * S, 0.f);
  const float special[] = {INFINITY, -INFINITY, NAN, 0.5f, nextafterf(0.5f, 1.f), nextafterf(0.5f, 0.f)};
  for (size_t i = 0; i < a.size(); ++i) {
    const unsigned r = (unsigned)((i + 1) * 2654435761u) >> 8, q = (unsigned)((i + 77) * 2246822519u) >> 8;
    a[i] = r % 11 == 0 ? special[(r / 11) % 6] : (float)(r % 4096) / 2048.f - 0.5f;
    b[i] = q % 13 == 0 ? special[(q / 13) % 6] : (float)(q % 4096) / 2048.f - 0.5f;
    pa[(i / W) * S + i % W] = a[i];
    pb[(i / W) * S + i % W] = b[i];
  }
  const std::vector<int64_t> s = sums_of(a, b, H, W), same = sums_of(a, a, H, W), padded = sums_of(pa, pb, S, S);
  int bad = s.empty() || same.empty() || padded.empty();
  if (!bad) {
    bad += s != padded;
    for (int l = 0; l <= n; ++l) bad += same[l * 3] != 0 || same[l * 3 + 1] != same[l * 3 + 2] || same[l * 3 + 1] != s[l * 3 + 1];
    int64_t sa = 0, sb = 0;                                              // the top level squares the two mask counts
    for (size_t i = 0; i < a.size(); ++i) { sa += a[i] > 0.5f; sb += b[i] > 0.5f; }
    bad += s[n * 3] != (sb - sa) * (sb - sa) || s[n * 3 + 1] != sa * sa || s[n * 3 + 2] != sb * sb || s[1] != sa || s[2] != sb;
  }
  const int C = DG_EOF_MAX_C;
  const dg_iscale_spec big = spec_of(C, true, DG_ISCALE_MAX_THR);
  std::vector<float> xa((size_t)C * H * W), xb(xa.size());
  for (size_t i = 0; i < xa.size(); ++i) { xa[i] = a[i % a.size()] * (1 + i / a.size()); xb[i] = b[i % b.size()]; }
  std::vector<int64_t> out((size_t)DG_HIST_MAX_OUT * DG_ISCALE_MAX_THR * (n + 1) * 3, 0);
  bad += dg_iscale_host(&big, xa.data(), xb.data(), C, H, W, out.data()) != DG_OK;
  return report("random pair", H, W, bad);
}

int main() {
  int bad = 0;
  bad += block(32, 32, 0, 7, 9) + block(32, 32, 2, 4, 28) + block(32, 32, 5, 0, 0) + block(20, 37, 3, 8, 24) + block(1, 2048, 0, 0, 2047);
  bad += checkerboard(2) + checkerboard(16) + checkerboard(64);
  const int grids[][2] = {{1, 1}, {1, 70}, {70, 1}, {5, 3}, {65, 33}, {3, 2048}, {2048, 2}};
  for (const auto& g : grids) bad += constant(g[0], g[1], 1.f) + constant(g[0], g[1], NAN) + random_pair(g[0], g[1]);
  // rejected arguments return a status and touch nothing
  const dg_iscale_spec s = spec_of(1, false, 1);
  dg_iscale_spec none = s;
  none.nthr = 0;
  std::vector<float> x(4, 0.f);
  std::vector<int64_t> out(2 * 3, 0);
  bad += dg_iscale_host(&none, x.data(), x.data(), 1, 2, 2, out.data()) == DG_OK;
  bad += dg_iscale_host(&s, x.data(), x.data(), 1, 0, 2, out.data()) == DG_OK;
  bad += dg_iscale_host(&s, x.data(), x.data(), 1, 2, 2049, out.data()) == DG_OK;
  bad += dg_iscale_host(&s, nullptr, x.data(), 1, 2, 2, out.data()) == DG_OK;
  bad += dg_iscale_levels(0, 1) != 0 || dg_iscale_levels(2048, 2048) != DG_ISCALE_MAX_LEVELS || dg_iscale_bound(2049, 1) != 0;
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
