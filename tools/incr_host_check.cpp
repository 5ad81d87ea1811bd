// Host memory-safety check of dg_incr_host (csrc/increments.hip): the host reference of the increment histograms on the shapes
// (1, 7, 13) and (3, 41, 37) with lags up to and beyond both extents, compiled with the address and undefined-behaviour
// sanitizers on the HOST side only and run on the CPU (no GPU is touched: dg_incr_host launches nothing).  Build and run from
// the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -c downgan_amd/csrc/increments.hip -o /tmp/incr_host_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o tools/incr_host_check \
//         tools/incr_host_check.cpp /tmp/incr_host_san.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
//   ./tools/incr_host_check
// The output arrays are allocated at exactly the size the contract states, so a write past a table is caught.
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#include "../include/downgan_hip.h"

static int run(int T, int C, int H, int W, bool speed, const std::vector<int>& lags, int nbins) {
  dg_incr_spec s{};
  s.speed_u = speed ? 0 : -1;
  s.speed_v = speed ? C - 1 : -1;
  s.nlag = (int)lags.size();
  s.nbins = nbins;
  const int nout = C + (speed ? 1 : 0);
  for (int l = 0; l < s.nlag; ++l) s.lag[l] = lags[l];
  for (int c = 0; c < C; ++c) { s.scale[c] = 0.5f + c; s.offset[c] = 0.25f * c; }
  for (int j = 0; j < nout; ++j)
    for (int l = 0; l < s.nlag; ++l) { s.lo[j][l] = -2.f; s.inv_w[j][l] = nbins / 4.f; }
  const size_t rows = (size_t)nout * 2 * s.nlag;
  std::vector<int64_t> counts(rows * (nbins + 3), 0), finite(rows, 0);
  std::vector<double> moments(rows * 6, 0.0);
  std::vector<float> x((size_t)C * H * W);
  long long total = 0;
  for (int t = 0; t < T; ++t) {
    for (size_t i = 0; i < x.size(); ++i) {
      const unsigned k = (unsigned)(i * 2654435761u + t * 40503u) >> 8;
      x[i] = k % 97 == 0 ? INFINITY : k % 89 == 0 ? NAN : k % 83 == 0 ? -INFINITY : (float)(k % 1024) / 256.f - 2.f;
    }
    const int rc = dg_incr_host(&s, x.data(), C, H, W, counts.data(), finite.data(), moments.data());
    if (rc != DG_OK) { printf("dg_incr_host failed: %d\n", rc); return 1; }
  }
  for (int64_t v : counts) total += v;
  long long want = 0;
  for (int l = 0; l < s.nlag; ++l)
    want += (long long)T * nout * ((long long)H * (W > lags[l] ? W - lags[l] : 0) + (long long)(H > lags[l] ? H - lags[l] : 0) * W);
  printf("T %d C %d H %d W %d nlag %d nbins %d: %lld increments (expected %lld)\n", T, C, H, W, s.nlag, nbins, total, want);
  return total == want ? 0 : 1;
}

int main() {
  int bad = 0;
  bad += run(1, 2, 7, 13, true, {1, 6, 7, 12, 13, 14, 255, 256}, 512);
  bad += run(3, 2, 41, 37, true, {1, 2, 36, 37, 40, 41, 42, 256}, 64);
  bad += run(1, 8, 7, 13, true, {3, 200}, 1);
  bad += run(3, 1, 41, 37, false, {256}, 7);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
