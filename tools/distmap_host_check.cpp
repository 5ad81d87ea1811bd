// Host memory-safety check of dg_distmap_host (csrc/distmap.hip): the host reference of the distance maps on planted fields (empty,
// full, one pixel in each corner, a NaN field, pseudo-random values next to +-inf and NaN) on the grids 1 x 1, 1 x W, H x 1, a
// ragged one and W = 2048, compiled with the address and undefined-behaviour sanitizers on the HOST side only and run on the CPU (no
// GPU is touched: the function launches nothing).  Every pair is also run with each output alone, which must give the same bytes,
// and the one-series call must give side 0 of the pair's d2.  Build and run from the repository root:
//   mkdir -p build
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -c downgan_amd/csrc/distmap.hip -o build/distmap_host_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o build/distmap_host_check \
//         tools/distmap_host_check.cpp build/distmap_host_san.o -L$ROCM_PATH/lib -lamdhip64 -Wl,-rpath,$ROCM_PATH/lib
//   ./build/distmap_host_check
// The arrays are allocated at exactly the size the contract states, so a read or write past one is caught.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../include/downgan_hip.h"

enum Plant { EMPTY, FULL, CORNERS, NANS, RANDOM };
static const char* const kNames[] = {"empty", "full", "corners", "nan", "random"};

static std::vector<float> plant(Plant what, int C, int H, int W, unsigned seed) {
  const size_t P = (size_t)H * W;
  std::vector<float> x((size_t)C * P, what == FULL ? 3.f : what == NANS ? NAN : -3.f);
  if (what == CORNERS)
    for (int c = 0; c < C; ++c) x[c * P] = x[c * P + W - 1] = x[c * P + P - W] = x[c * P + P - 1] = 3.f;
  if (what == RANDOM) {
    const float special[] = {INFINITY, -INFINITY, NAN, 1.f, 2.f, nextafterf(1.f, 2.f), nextafterf(2.f, 3.f)};
    for (size_t i = 0; i < x.size(); ++i) {
      const unsigned r = (unsigned)((i + seed) * 2654435761u) >> 8;
      x[i] = r % 11 == 0 ? special[(r / 11) % 7] : (float)(r % 4096) / 512.f - 5.f;
    }
  }
  return x;
}

template <typename V> static bool same(const std::vector<V>& a, const std::vector<V>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0;
}

static int run(int C, int H, int W, bool speed, int nthr, int nring, int cutoff, Plant pa, Plant pb) {
  dg_distmap_spec s{};
  s.speed_u = speed ? 0 : -1;
  s.speed_v = speed ? C - 1 : -1;
  s.nthr = nthr; s.nring = nring; s.cutoff = cutoff;
  const int nout = C + (speed ? 1 : 0);
  const float thr[DG_DIST_MAX_THR] = {1.f, 2.f, -1.f, 0.f};
  for (int c = 0; c < C; ++c) { s.scale[c] = 1.5f; s.offset[c] = -0.25f; }
  for (int j = 0; j < nout; ++j)
    for (int k = 0; k < nthr; ++k) s.thr[j][k] = thr[k];
  const size_t P = (size_t)H * W, njk = (size_t)nout * nthr, nb = (size_t)nring + 2;
  const std::vector<float> a = plant(pa, C, H, W, 1), b = plant(pb, C, H, W, 77);
  std::vector<int64_t> rec(njk * DG_DIST_COLS, -7), rings(njk * 2 * nb, 0), rec1(rec), rings1(rings);
  std::vector<int32_t> d2(2 * njk * P, -7), d2only(d2), one(2 * njk * P, -7);
  int rc = dg_distmap_host(&s, a.data(), b.data(), C, H, W, rec.data(), rings.data(), d2.data());
  if (rc == DG_OK) rc = dg_distmap_host(&s, a.data(), b.data(), C, H, W, rec1.data(), nullptr, nullptr);
  if (rc == DG_OK) rc = dg_distmap_host(&s, a.data(), b.data(), C, H, W, nullptr, rings1.data(), nullptr);
  if (rc == DG_OK) rc = dg_distmap_host(&s, a.data(), b.data(), C, H, W, nullptr, nullptr, d2only.data());
  if (rc == DG_OK) rc = dg_distmap_host(&s, a.data(), nullptr, C, H, W, nullptr, nullptr, one.data());
  if (rc != DG_OK) { printf("dg_distmap_host failed: %d\n", rc); return 1; }
  int bad = 0;
  bad += !same(rec, rec1) || !same(rings, rings1) || !same(d2, d2only);
  bad += memcmp(one.data(), d2.data(), njk * P * sizeof(int32_t)) != 0;                 // side 0 alone
  for (size_t i = njk * P; i < one.size(); ++i) bad += one[i] != -7;                    // side 1 untouched
  long long pixels = 0, ringed = 0;
  for (size_t r = 0; r < njk; ++r) {
    const int64_t* v = &rec[r * DG_DIST_COLS];
    pixels += v[0] + v[1];
    const bool both = v[0] > 0 && v[1] > 0;
    for (int c = 3; c <= 8; ++c) bad += both ? v[c] < 0 : v[c] != -1;
    bad += v[2] > v[0] || v[2] > v[1] || v[9] < 0 || v[10] < v[9];
    for (int side = 0; side < 2; ++side)                                                 // an empty mask: FAR everywhere
      if (v[side] == 0)
        for (size_t p = 0; p < P; ++p) bad += d2[(side * njk + r) * P + p] != DG_DIST_FAR;
  }
  for (int64_t v : rings) ringed += v;
  bad += ringed != pixels;                                                               // every set pixel is in exactly one bin
  printf("C %d %4d x %4d speed %d nthr %d nring %3d cutoff %3d %-7s vs %-7s: %lld set pixels, %lld in rings, %s\n", C, H, W, (int)speed,
         nthr, nring, cutoff, kNames[pa], kNames[pb], pixels, ringed, bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}

int main() {
  const Plant all[] = {EMPTY, FULL, CORNERS, NANS, RANDOM};
  const int grids[][2] = {{1, 1}, {1, 70}, {70, 1}, {5, 67}, {3, 2048}, {2048, 2}};
  int bad = 0;
  for (const auto& g : grids)
    for (Plant pa : all)
      for (Plant pb : all) bad += run(2, g[0], g[1], true, 2, 9, 6, pa, pb);
  bad += run(1, 9, 13, false, 1, 1, 1, RANDOM, CORNERS);                                 // the smallest spec
  bad += run(8, 6, 7, true, 4, 128, 512, RANDOM, RANDOM);                                // the largest
  bad += run(3, 1, 2048, false, 4, 128, 512, CORNERS, EMPTY);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
