// Host memory-safety check of dg_qmap_fit_host and dg_qmap_apply_host (csrc/qmap.hip): the two host references of empirical
// quantile mapping on planted tables (a pixel empty on both sides, one side empty, all mass in the underflow, the overflow and the
// NaN row, a single non-empty bin on either side, a == b with empty bins inside, 2^26 - 1 counts in one bin against a spread-out
// other side, sparse pseudo-random counts) and planted values (every bin edge and its fp32 neighbours, +-0, denormals, +-inf, NaN,
// +-FLT_MAX) for bins = 1, bins = 64 with an affine transform and the speed, and bins = 256 without, compiled with the address and
// undefined-behaviour sanitizers on the HOST side only and run on the CPU (no GPU is touched: neither function launches
// anything).  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -c downgan_amd/csrc/qmap.hip -o /tmp/qmap_host_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o tools/qmap_host_check \
//         tools/qmap_host_check.cpp /tmp/qmap_host_san.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
//   ./tools/qmap_host_check
// The arrays are allocated at exactly the size the contract states, so a read or write past a table is caught.
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../include/downgan_hip.h"

static int run(int T, int C, int P, bool speed, int nbins, float lo, float hi, float scale, float offset) {
  dg_hist_spec s{};
  s.nbins = nbins;
  s.speed_u = speed ? 0 : -1;
  s.speed_v = speed ? 1 : -1;
  const int nout = C + (speed ? 1 : 0), nb3 = nbins + 3, fin = nbins + 2;
  std::vector<float> lov(nout);
  std::vector<double> wv(nout);
  for (int c = 0; c < C; ++c) { s.scale[c] = scale; s.offset[c] = offset; }
  for (int j = 0; j < nout; ++j) {
    lov[j] = j < C ? lo : 0.f;
    wv[j] = (j < C ? (double)hi - lo : 2.0 * hi) / nbins;
    s.lo[j] = lov[j];
    s.inv_w[j] = (float)(1.0 / wv[j]);
  }
  // the planted table: pixel p carries pattern p % 12
  std::vector<int32_t> counts((size_t)nout * 2 * nb3 * P, 0);
  uint32_t seed = 12345u + (uint32_t)nbins;
  auto rnd = [&](uint32_t n) { seed = seed * 1664525u + 1013904223u; return (int32_t)((seed >> 8) % n); };
  for (int j = 0; j < nout; ++j)
    for (int p = 0; p < P; ++p) {
      int32_t* real = counts.data() + ((size_t)j * 2 * nb3) * P + p;
      int32_t* gen = real + (size_t)nb3 * P;
      auto at = [&](int32_t* col, int r) -> int32_t& { return col[(size_t)r * P]; };
      const int k = p % 12, one = 1 + (p + j) % nbins;
      switch (k) {
        case 0: break;
        case 1: for (int r = 0; r < fin; ++r) at(gen, r) = rnd(6); at(gen, 1) += 1; break;
        case 2: for (int r = 0; r < fin; ++r) at(real, r) = rnd(6); at(real, 1) += 1; break;
        case 3: at(real, 0) = 5 + j; at(gen, 0) = 9; break;
        case 4: at(real, nbins + 1) = 3; at(gen, nbins + 1) = 4 + j; break;
        case 5: at(real, nbins + 2) = 7; at(gen, nbins + 2) = 8; break;
        case 6: at(real, one) = 11; for (int r = 0; r < fin; ++r) at(gen, r) = rnd(9); at(gen, nbins) += 1; break;
        case 7: at(gen, one) = 11; for (int r = 0; r < fin; ++r) at(real, r) = rnd(9); at(real, nbins) += 1; break;
        case 8: for (int r = 0; r < fin; ++r) at(real, r) = at(gen, r) = rnd(50) * rnd(2); at(real, one) += 3; at(gen, one) += 3; break;
        case 9: at(gen, one) = (1 << 26) - 1; for (int r = 0; r < fin; ++r) at(real, r) = ((1 << 26) - 1) / fin - rnd(1000); break;
        case 10: at(real, one) = (1 << 26) - 1; for (int r = 0; r < fin; ++r) at(gen, r) = ((1 << 26) - 1) / fin - rnd(1000); break;
        default: for (int r = 0; r < fin; ++r) { at(real, r) = rnd(1000) * rnd(2); at(gen, r) = rnd(1000) * rnd(2); } break;
      }
      if (k != 5) { at(real, nbins + 2) = rnd(50); at(gen, nbins + 2) = rnd(50); }
    }
  std::vector<float> nodes((size_t)nout * nb3 * P, -77.f);
  int rc = dg_qmap_fit_host(counts.data(), nout, nbins, P, lov.data(), wv.data(), nodes.data());
  if (rc != DG_OK) { printf("dg_qmap_fit_host failed: %d\n", rc); return 1; }
  int bad = 0;
  for (int j = 0; j < nout; ++j)
    for (int p = 0; p < P; ++p) {
      const float* o = nodes.data() + (size_t)j * nb3 * P + p;
      for (int k = 0; k <= nbins; ++k) {
        bad += !(o[(size_t)k * P] == o[(size_t)k * P]);                                        // no NaN
        if (k) bad += o[(size_t)k * P] < o[(size_t)(k - 1) * P];                                // monotone
      }
      const int k = p % 12;
      if (k == 0 || k == 1 || k == 2 || k == 5 || k == 8)                                         // the identity
        for (int e = 0; e <= nbins; ++e) bad += o[(size_t)e * P] != (float)((double)lov[j] + e * wv[j]);
    }
  // planted values: every edge and its neighbours in input units, then the specials, then a ramp
  std::vector<float> sv;
  for (int k = 0; k <= nbins; ++k) {
    const float e = (float)((((double)lo + k * ((double)hi - lo) / nbins) - offset) / scale);
    sv.push_back(e); sv.push_back(nextafterf(e, -INFINITY)); sv.push_back(nextafterf(e, INFINITY));
  }
  const float special[] = {0.f, -0.f, 1e-45f, -1e-45f, 3e-39f, -3e-39f, FLT_MIN, -FLT_MIN, INFINITY, -INFINITY, NAN, FLT_MAX, -FLT_MAX,
                           (3.f - offset) / scale, (4.f - offset) / scale};
  for (float v : special) sv.push_back(v);
  std::vector<float> x((size_t)T * C * P), out((size_t)T * nout * P, -77.f);
  for (size_t i = 0; i < x.size(); ++i) x[i] = sv[(i * 11 + 3) % sv.size()];                      // 11 is prime to every sv.size() below
  for (size_t i = sv.size(); i < x.size(); i += 3) x[i] = (float)((i * 2654435761u >> 8) % 2048) / 256.f - 4.f;
  rc = dg_qmap_apply_host(&s, x.data(), C, T, P, nodes.data(), out.data());
  if (rc != DG_OK) { printf("dg_qmap_apply_host failed: %d\n", rc); return 1; }
  long long nans = 0, nan_in = 0;
  for (size_t i = 0; i < out.size(); ++i) {
    uint32_t b;
    memcpy(&b, &out[i], 4);
    if (out[i] != out[i]) { ++nans; bad += b != 0x7fc00000u; }
  }
  for (int t = 0; t < T; ++t)
    for (int p = 0; p < P; ++p) {
      bool any = false;
      for (int c = 0; c < C; ++c) {
        const float v = x[((size_t)t * C + c) * P + p];
        if (v != v) { ++nan_in; any |= c < 2; }                                                  // the speed reads channels 0 and 1
        if (std::isinf(v) && (scale > 0) == (v > 0) && !speed) bad += out[((size_t)t * nout + c) * P + p] != INFINITY;
      }
      if (speed && any) ++nan_in;
    }
  bad += nans != nan_in;
  printf("T %d C %d P %d speed %d nbins %d: %lld NaN out of %lld NaN in, %s\n", T, C, P, (int)speed, nbins, nans, nan_in, bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}

int main() {
  int bad = 0;
  bad += run(1, 2, 7 * 13, false, 1, -1.f, 1.f, 1.f, 0.f);
  bad += run(5, 2, 40 * 37, true, 64, -8.f, 8.f, 2.f, -1.f);
  bad += run(3, 2, 16 * 16, false, 256, -4.f, 4.f, 1.f, 0.f);
  bad += run(3, 8, 5, true, 256, -8.f, 8.f, 0.5f, 0.25f);
  bad += run(2, 1, 1, false, 7, 0.f, 1.f, 1.f, 0.f);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
