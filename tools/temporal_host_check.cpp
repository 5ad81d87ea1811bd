// Host memory-safety check of dg_temporal_host (csrc/temporal.hip): the host reference of the temporal diagnostics on planted data
// (values at every threshold and their fp32 neighbours, +-0, denormals, +-inf, NaN, +-FLT_MAX, a pixel that is never finite, a
// spell longer than ndur, a series shorter than the largest lag), compiled with the address and undefined-behaviour sanitizers on
// the HOST side only and run on the CPU (no GPU is touched: the function launches nothing).  Every series is fed in one call and
// in chunks of one field, and the two must give the same bytes in all seven arrays.  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -c downgan_amd/csrc/temporal.hip -o /tmp/temporal_host_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o tools/temporal_host_check \
//         tools/temporal_host_check.cpp /tmp/temporal_host_san.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
//   ./tools/temporal_host_check
// The arrays are allocated at exactly the size the contract states, so a read or write past one is caught.
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../include/downgan_hip.h"

struct State {
  std::vector<int32_t> open, spellmap, accnt;
  std::vector<float> tail;
  std::vector<int64_t> spells, ramps;
  std::vector<double> acsum;
  State(const dg_temporal_spec& s, int nout, int P) {
    const size_t R = s.nlag ? s.lag[s.nlag - 1] : 0, o = nout, p = P;
    open.assign(o * s.nthr * p, 0);
    tail.assign(o * R * p, 0.f);
    spells.assign(o * s.nthr * s.ndur, 0);
    spellmap.assign(o * s.nthr * 3 * p, 0);
    ramps.assign(o * s.nlag * (s.nbins + 3), 0);
    acsum.assign(o * (2 + 2 * s.nlag) * p, 0.0);
    accnt.assign(o * (1 + s.nlag) * p, 0);
  }
  template <typename V> static V* ptr(std::vector<V>& v) { return v.empty() ? nullptr : v.data(); }   // an absent array is NULL
  int add(const dg_temporal_spec& s, const float* x, int C, int T, int P, int64_t t0) {
    return dg_temporal_host(&s, x, C, T, P, t0, ptr(open), ptr(tail), ptr(spells), ptr(spellmap), ptr(ramps), ptr(acsum), ptr(accnt));
  }
  template <typename V> static bool same(const std::vector<V>& a, const std::vector<V>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
  }
  bool equals(const State& b) const {
    return same(open, b.open) && same(tail, b.tail) && same(spells, b.spells) && same(spellmap, b.spellmap) && same(ramps, b.ramps) &&
           same(acsum, b.acsum) && same(accnt, b.accnt);
  }
};

static int run(int T, int C, int P, bool speed, int nthr, int ndur, int nlag, const int* lags, int nbins, float scale, float offset) {
  dg_temporal_spec s{};
  s.speed_u = speed ? 0 : -1;
  s.speed_v = speed ? 1 : -1;
  s.nthr = nthr; s.ndur = ndur; s.nlag = nlag; s.nbins = nbins;
  const int nout = C + (speed ? 1 : 0);
  const float thr[DG_TEMPORAL_MAX_THR] = {1.f, 2.f, -1.f, -2.f};
  for (int k = 0; k < nthr; ++k) s.below[k] = k >= 2;
  for (int l = 0; l < nlag; ++l) s.lag[l] = lags[l];
  for (int c = 0; c < C; ++c) { s.scale[c] = scale; s.offset[c] = offset; }
  for (int j = 0; j < nout; ++j) {
    for (int k = 0; k < nthr; ++k) s.thr[j][k] = thr[k];
    for (int l = 0; l < nlag; ++l) { s.lo[j][l] = -4.f; s.inv_w[j][l] = (float)(nbins / 8.0); }
  }
  // planted: every threshold and its neighbours in input units, then the specials; pixel P - 1 of channel 0 is never finite;
  // pixel 0 of every channel stays above every "above" threshold for min(T, ndur + 3) fields: a spell longer than ndur
  std::vector<float> sv;
  for (int k = 0; k < nthr; ++k) {
    const float e = (thr[k] - offset) / scale;
    sv.push_back(e); sv.push_back(nextafterf(e, -INFINITY)); sv.push_back(nextafterf(e, INFINITY));
  }
  const float special[] = {0.f, -0.f, 1e-45f, -1e-45f, 3e-39f, -3e-39f, FLT_MIN, -FLT_MIN, INFINITY, -INFINITY, NAN, FLT_MAX, -FLT_MAX};
  for (float v : special) sv.push_back(v);
  std::vector<float> x((size_t)T * C * P);
  for (size_t i = 0; i < x.size(); ++i) x[i] = (i % 3 == 1) ? sv[(i / 3) % sv.size()] : (float)((i * 2654435761u >> 8) % 2048) / 256.f - 4.f;
  for (int t = 0; t < T; ++t) {
    x[((size_t)t * C) * P + P - 1] = NAN;
    if (t < ndur + 3 && P > 1)
      for (int c = 0; c < C; ++c) x[((size_t)t * C + c) * P] = (50.f - offset) / scale;
  }
  State one(s, nout, P), many(s, nout, P);
  int rc = one.add(s, x.data(), C, T, P, 0);
  for (int t = 0; t < T && rc == DG_OK; ++t) rc = many.add(s, x.data() + (size_t)t * C * P, C, 1, P, t);
  if (rc != DG_OK) { printf("dg_temporal_host failed: %d\n", rc); return 1; }
  int bad = one.equals(many) ? 0 : 1;
  long long ramps = 0, want = 0, never = 0;
  for (int64_t v : one.ramps) ramps += v;
  for (int l = 0; l < nlag; ++l) want += (long long)(T > lags[l] ? T - lags[l] : 0) * nout * P;
  bad += ramps != want;
  never = one.accnt[(size_t)P - 1];                                   // channel 0, row n, the never-finite pixel
  bad += never != 0;
  if (nthr > 0 && P > 1 && T >= ndur + 3)                              // the planted long spell: length ndur + 3 or more
    bad += one.spellmap[2 * (size_t)P] < ndur + 3;                      // channel 0, threshold 0, row 2 (longest), pixel 0
  printf("T %d C %d P %d speed %d nthr %d ndur %d nlag %d nbins %d: %lld ramps (expected %lld), chunks of 1 %s, %s\n", T, C, P, (int)speed,
         nthr, ndur, nlag, nbins, ramps, want, one.equals(many) ? "equal" : "DIFFER", bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}

int main() {
  const int l4[] = {1, 2, 3, 24}, l1[] = {1}, l2[] = {5, 24};
  int bad = 0;
  bad += run(40, 2, 7 * 13, true, 4, 8, 4, l4, 16, 2.f, -1.f);
  bad += run(50, 1, 1, false, 1, 1, 0, l1, 1, 1.f, 0.f);               // no lag: tail and ramps are NULL
  bad += run(30, 2, 35, false, 0, 8, 1, l1, 1, 1.f, 0.f);              // no threshold: open, spells and spellmap are NULL
  bad += run(7, 3, 16, true, 2, 256, 2, l2, 512, 0.5f, 0.25f);         // a series shorter than the largest lag
  bad += run(1, 8, 5, true, 4, 4, 4, l4, 512, 1.f, 0.f);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
