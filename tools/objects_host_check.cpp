// Host memory-safety check of dg_objects_host (csrc/objects.hip): the host reference of the exceedance objects on planted fields
// (empty, full, checkerboard, serpentine, pseudo-random masks; values at the threshold and its fp32 neighbours, +-0, denormals,
// +-inf, NaN, +-FLT_MAX, saturating intensities), compiled with the address and undefined-behaviour sanitizers on the HOST side
// only and run on the CPU (no GPU is touched: the function launches nothing).  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -c downgan_amd/csrc/objects.hip -o build/objects_host_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o build/objects_host_check \
//         tools/objects_host_check.cpp build/objects_host_san.o -L$ROCM_PATH/lib -lamdhip64 -Wl,-rpath,$ROCM_PATH/lib
//   ./build/objects_host_check
// The tables are allocated at exactly `capacity` rows (heap blocks of that size, none when capacity is 0), count > capacity
// included, and per_plane at exactly 2 nout nthr entries: a write past either is caught.  Every case is also run with too small
// a table, which must leave the count, per_plane and the leading rows unchanged.
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../include/downgan_hip.h"

static dg_objects_spec make_spec(int C, bool speed, int nthr, int conn, float inv_quantum, float scale, float offset) {
  dg_objects_spec s{};
  s.speed_u = speed ? 0 : -1;
  s.speed_v = speed ? 1 : -1;
  s.nthr = nthr; s.connectivity = conn; s.inv_quantum = inv_quantum;
  const float thr[DG_OBJ_MAX_THR] = {1.f, 2.f, -1.f, 0.f};
  for (int c = 0; c < C; ++c) { s.scale[c] = scale; s.offset[c] = offset; }
  for (int j = 0; j < C + (speed ? 1 : 0); ++j)
    for (int k = 0; k < nthr; ++k) s.thr[j][k] = thr[k];
  return s;
}

// one call with a table of exactly `cap` rows; returns the count, fills rows (the leading min(count, cap)) and per_plane
static int call(const dg_objects_spec& s, const float* a, const float* b, int C, int H, int W, int64_t cap, int64_t* count,
                std::vector<int64_t>* rows, std::vector<int64_t>* per_plane) {
  const int nout = C + (s.speed_u >= 0 ? 1 : 0);
  int64_t* table = cap ? new int64_t[(size_t)cap * DG_OBJ_COLS] : nullptr;      // exactly capacity rows
  int64_t* pp = new int64_t[(size_t)2 * nout * s.nthr];
  const int rc = dg_objects_host(&s, a, b, C, H, W, table, cap, count, pp);
  if (rc == DG_OK) {
    const int64_t n = *count < cap ? *count : cap;
    rows->assign(table, table + n * DG_OBJ_COLS);
    per_plane->assign(pp, pp + 2 * nout * s.nthr);
  }
  delete[] table;
  delete[] pp;
  return rc;
}

static int run(const char* name, int C, int H, int W, bool speed, int nthr, int conn, bool paired, int pattern) {
  const dg_objects_spec s = make_spec(C, speed, nthr, conn, pattern == 5 ? 1024.f : 16.f, 2.f, -1.f);
  const size_t P = (size_t)H * W;
  const float special[] = {1.f, nextafterf(1.f, 0.f), nextafterf(1.f, 2.f), 0.f, -0.f, 1e-45f, -3e-39f, FLT_MIN, INFINITY, -INFINITY,
                           NAN, FLT_MAX, -FLT_MAX, 1.5f, 0.5f};
  const size_t nspecial = sizeof(special) / sizeof(special[0]);
  std::vector<float> x[2];
  for (int e = 0; e < 2; ++e) {
    x[e].resize((size_t)C * P);
    for (int c = 0; c < C; ++c) {
      for (int h = 0; h < H; ++h) {
        for (int w = 0; w < W; ++w) {
          const size_t i = (size_t)c * P + (size_t)h * W + w;
          bool set = false;
          switch ((pattern + c + e) % 5) {
            case 0: set = false; break;
            case 1: set = true; break;
            case 2: set = (h + w) % 2 == 0; break;
            case 3: set = h % 2 == 0 || (h % 4 == 1 && w == W - 1) || (h % 4 == 3 && w == 0); break;
            default: set = ((i * 2654435761u) >> 13) % 100 < 59; break;
          }
          float y = set ? 1.25f + (float)((i * 40503u) % 64) / 32.f : -3.f + (float)((i * 9973u) % 64) / 20.f;   // output units
          if (pattern == 5 && set) y = 1e30f;                                   // saturating intensities
          if (pattern == 4 && i % 7 == 3) y = special[(i / 7) % nspecial];
          x[e][i] = (y - s.offset[c]) / s.scale[c];
        }
      }
    }
  }
  const float* b = paired ? x[1].data() : nullptr;
  int64_t count = -1, c2 = -1;
  std::vector<int64_t> none, all, pp0, pp1, some;
  int rc = call(s, x[0].data(), b, C, H, W, 0, &count, &none, &pp0);             // capacity 0: table NULL, count only
  if (rc != DG_OK || count < 0) { printf("%s: dg_objects_host failed: %d\n", name, rc); return 1; }
  rc = call(s, x[0].data(), b, C, H, W, count, &c2, &all, &pp1);                 // exactly count rows
  int bad = rc != DG_OK || c2 != count || pp0 != pp1 || (int64_t)all.size() != count * DG_OBJ_COLS;
  const int64_t caps[] = {1, count / 2, count - 1};
  for (int64_t cap : caps) {
    if (cap < 1 || cap >= count) continue;
    rc = call(s, x[0].data(), b, C, H, W, cap, &c2, &some, &pp1);                // count > capacity: nothing past the end
    bad += rc != DG_OK || c2 != count || pp0 != pp1 || (int64_t)some.size() != cap * DG_OBJ_COLS ||
           memcmp(some.data(), all.data(), some.size() * sizeof(int64_t)) != 0;
  }
  int64_t total = 0, area = 0;
  for (int64_t v : pp0) total += v;
  bad += total != count;
  for (int64_t r = 0; r < count; ++r) {                                          // sorted by (plane, root), boxes inside the grid
    const int64_t* v = all.data() + r * DG_OBJ_COLS;
    area += v[2];
    bad += v[2] < 1 || v[8] < 0 || v[9] >= H || v[10] < 0 || v[11] >= W || v[8] > v[9] || v[10] > v[11] || v[1] / W != v[8] ||
           v[7] > 16777215 || v[4] > v[2] * 16777215 || v[3] > v[2] || (!paired && v[3] != 0);
    if (r > 0) bad += !(v[-DG_OBJ_COLS] < v[0] || (v[-DG_OBJ_COLS] == v[0] && v[1 - DG_OBJ_COLS] < v[1]));
  }
  printf("%s: C %d %d x %d speed %d nthr %d conn %d paired %d: %lld objects, %lld pixels, %s\n", name, C, H, W, (int)speed, nthr, conn,
         (int)paired, (long long)count, (long long)area, bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}

int main() {
  int bad = 0;
  bad += run("zoo 8", 2, 33, 67, true, 2, 8, true, 0);
  bad += run("zoo 4", 2, 33, 67, true, 2, 4, true, 1);
  bad += run("shifted", 3, 20, 21, true, 4, 8, true, 2);
  bad += run("one series", 2, 17, 130, false, 3, 4, false, 3);
  bad += run("specials", 1, 40, 9, false, 4, 8, true, 4);
  bad += run("saturating", 1, 64, 64, false, 1, 4, true, 5);
  bad += run("one pixel", 1, 1, 1, false, 1, 8, true, 1);
  bad += run("one row", 8, 1, 300, true, 2, 8, true, 3);
  bad += run("one column", 1, 300, 1, false, 2, 4, false, 2);
  dg_objects_spec s = make_spec(1, false, 1, 6, 1.f, 1.f, 0.f);                  // rejected: nothing is read or written
  int64_t count = 0, pp[2] = {0, 0};
  const float v = 0.f;
  bad += dg_objects_host(&s, &v, nullptr, 1, 1, 1, nullptr, 0, &count, pp) != DG_ERR_BAD_SHAPE;
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
