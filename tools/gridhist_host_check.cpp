// Host memory-safety check of dg_gridhist_host and dg_gridhist_scan_host (csrc/gridhist.hip): the two host references of the
// per-gridpoint histograms on planted data (every bin edge and its fp32 neighbours, +-0, denormals, +-inf, NaN, +-FLT_MAX, (3, 4)
// pairs, one pixel that is never finite) for bins = 1, bins = 64 with an affine transform and the speed, and bins = 256 without,
// compiled with the address and undefined-behaviour sanitizers on the HOST side only and run on the CPU (no GPU is touched:
// neither function launches anything).  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -c downgan_amd/csrc/gridhist.hip -o /tmp/gridhist_host_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o tools/gridhist_host_check \
//         tools/gridhist_host_check.cpp /tmp/gridhist_host_san.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
//   ./tools/gridhist_host_check
// The arrays are allocated at exactly the size the contract states, so a read or write past a table is caught.
#include <float.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#include "../include/downgan_hip.h"

static int run(int T, int C, int P, bool speed, int nbins, float lo, float hi, float scale, float offset, bool paired) {
  dg_hist_spec s{};
  s.nbins = nbins;
  s.speed_u = speed ? 0 : -1;
  s.speed_v = speed ? 1 : -1;
  const int nout = C + (speed ? 1 : 0), S = paired ? 2 : 1, nb3 = nbins + 3;
  for (int c = 0; c < C; ++c) { s.scale[c] = scale; s.offset[c] = offset; }
  for (int j = 0; j < nout; ++j) { s.lo[j] = j < C ? lo : 0.f; s.inv_w[j] = (float)((double)nbins / (j < C ? (double)hi - lo : 2.0 * hi)); }
  // planted: every edge and its neighbours in input units, then the specials, then a ramp; pixel P - 1 of channel 0 never finite
  std::vector<float> sv;
  for (int k = 0; k <= nbins; ++k) {
    const float e = (float)((((double)lo + k * ((double)hi - lo) / nbins) - offset) / scale);
    sv.push_back(e); sv.push_back(nextafterf(e, -INFINITY)); sv.push_back(nextafterf(e, INFINITY));
  }
  const float special[] = {0.f, -0.f, 1e-45f, -1e-45f, 3e-39f, -3e-39f, FLT_MIN, -FLT_MIN, INFINITY, -INFINITY, NAN, FLT_MAX, -FLT_MAX,
                           (3.f - offset) / scale, (4.f - offset) / scale};
  for (float v : special) sv.push_back(v);
  std::vector<float> xa((size_t)T * C * P), xb(paired ? xa.size() : 0);
  for (size_t i = 0; i < xa.size(); ++i) {
    xa[i] = i < sv.size() ? sv[i] : (float)((i * 2654435761u >> 8) % 2048) / 256.f - 4.f;
    if (paired) xb[i] = sv[(i * 7 + 3) % sv.size()];
  }
  for (int t = 0; t < T; ++t) xa[((size_t)t * C) * P + P - 1] = NAN;
  std::vector<int32_t> counts((size_t)nout * S * nb3 * P, 0);
  for (int rep = 0; rep < 2; ++rep) {                                // accumulates: twice the fields
    const int rc = dg_gridhist_host(&s, xa.data(), paired ? xb.data() : nullptr, C, T, P, counts.data());
    if (rc != DG_OK) { printf("dg_gridhist_host failed: %d\n", rc); return 1; }
  }
  long long total = 0, never = 0;
  for (int32_t v : counts) total += v;
  for (int r = 0; r < nbins + 2; ++r) never += counts[(size_t)r * P + P - 1];                     // channel 0, side a, pixel P - 1
  const double q[DG_GRIDHIST_MAX_Q] = {0.5, 0.25, nextafter(0.25, 0.0), nextafter(0.25, 1.0), 1e-300, 0.01, 0.05, 0.1,
                                       0.3, 0.75, 0.9, 0.95, 0.98, 0.99, 0.999, nextafter(1.0, 0.0)};
  int bad = total != 2LL * T * nout * S * P || never != 0;
  const int nq[] = {1, 3, DG_GRIDHIST_MAX_Q};
  for (int Q : nq) {
    std::vector<int32_t> ranks((size_t)nout * S * Q * 3 * P, 7);
    std::vector<int64_t> dist(paired ? (size_t)nout * 2 * P : 0, 7);
    const int rc = dg_gridhist_scan_host(counts.data(), nout, S, nbins, P, q, Q, ranks.data(), paired ? dist.data() : nullptr);
    if (rc != DG_OK) { printf("dg_gridhist_scan_host failed: %d\n", rc); return 1; }
    for (size_t i = 0; i < ranks.size(); i += (size_t)3 * P)         // the row of every (j, s, q, p): -1 or 0 .. nbins + 1
      for (int p = 0; p < P; ++p) bad += ranks[i + p] < -1 || ranks[i + p] > nbins + 1 || (ranks[i + p] >= 0 && ranks[i + 2 * P + p] < 1);
    for (int64_t v : dist) bad += v < -1;
    bad += ranks[(size_t)P - 1] != -1;                               // the never-finite pixel
    if (paired) bad += dist[(size_t)P - 1] != -1;
  }
  printf("T %d C %d P %d speed %d nbins %d paired %d: %lld counts (expected %lld), %s\n", T, C, P, (int)speed, nbins, (int)paired, total,
         2LL * T * nout * S * P, bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}

int main() {
  int bad = 0;
  bad += run(1, 2, 7 * 13, false, 1, -1.f, 1.f, 1.f, 0.f, true);
  bad += run(5, 2, 40 * 37, true, 64, -8.f, 8.f, 2.f, -1.f, true);
  bad += run(3, 2, 16 * 16, false, 256, -4.f, 4.f, 1.f, 0.f, true);
  bad += run(3, 8, 5, true, 256, -8.f, 8.f, 0.5f, 0.25f, false);
  bad += run(2, 1, 1, false, 7, 0.f, 1.f, 1.f, 0.f, true);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
