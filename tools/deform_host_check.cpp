// Host memory-safety check of dg_deform_host / dg_deform_field_host (csrc/deform.hip): the host reference of the field-deformation
// sums on small and ragged grids (1 x 1, 1 x W, H x 1, sides that are no multiple of 2^F, levels that shrink to one pixel), F = 1 .. 4,
// with answers that hold by the definition (identical fields never move and leave no error; empty fields count nothing; the table
// sums to n_target; swapping the sides swaps the directions; the morphed field is the source read through the displacement; a
// pattern moved by a small vector well inside the grid is found), compiled with the address and undefined-behaviour sanitizers on
// the HOST side only and run on the CPU (no GPU is touched: the functions launch nothing).  Build and run from the repository root:
//   mkdir -p build
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -c downgan_amd/csrc/deform.hip -o build/deform_host_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o build/deform_host_check \
//         tools/deform_host_check.cpp build/deform_host_san.o -L$ROCM_PATH/lib -lamdhip64 -Wl,-rpath,$ROCM_PATH/lib
//   ./build/deform_host_check
// The arrays are allocated at exactly the size the contract states, so a read or write past one is caught.
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#include "../include/downgan_hip.h"

static dg_deform_spec spec_of(int C, bool speed, int levels) {
  dg_deform_spec s{};
  s.speed_u = speed ? 0 : -1;
  s.speed_v = speed ? C - 1 : -1;
  s.levels = levels;
  for (int c = 0; c < C; ++c) { s.scale[c] = 1.f; s.offset[c] = 0.f; }
  for (int j = 0; j < C + (speed ? 1 : 0); ++j) { s.lo[j] = 0.25f; s.inv_step[j] = 32.f; }
  return s;
}

static int max_disp(int F) { return 2 * ((2 << F) - 1); }

struct Out {
  int nout, side, H, W;
  std::vector<int64_t> disp, scal;
  std::vector<int16_t> field;
  std::vector<uint8_t> mor;
  bool ok;
};

// every output of one field pair, each array exactly as large as the contract states
static Out run(const dg_deform_spec& s, int C, const std::vector<float>& a, const std::vector<float>& b, int H, int W) {
  Out o;
  o.nout = C + (s.speed_u >= 0 ? 1 : 0);
  o.side = 2 * max_disp(s.levels) + 1;
  o.H = H; o.W = W;
  const size_t P = (size_t)H * W;
  o.disp.assign((size_t)o.nout * 2 * o.side * o.side, 0);
  o.scal.assign((size_t)o.nout * 2 * DG_DEFORM_SCALARS, 0);
  o.field.assign((size_t)o.nout * 2 * 2 * P, (int16_t)-777);
  o.mor.assign((size_t)o.nout * 2 * P, (uint8_t)99);
  o.ok = dg_deform_host(&s, a.data(), b.data(), C, H, W, o.disp.data(), o.scal.data()) == DG_OK &&
         dg_deform_field_host(&s, a.data(), b.data(), C, H, W, o.field.data(), o.mor.data()) == DG_OK;
  return o;
}

static int report(const char* what, int H, int W, int F, int bad) {
  printf("%-34s %4d x %4d F=%d: %s\n", what, H, W, F, bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}

// a smooth bump pattern, deterministic; (oy, ox) moves it
static std::vector<float> pattern(int C, int H, int W, int oy, int ox) {
  std::vector<float> x((size_t)C * H * W);
  for (int c = 0; c < C; ++c)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w) {
        const float y = (float)(h - oy), z = (float)(w - ox);
        x[((size_t)c * H + h) * W + w] = 3.f * std::sin(0.37f * y + 0.5f * c) * std::cos(0.29f * z - 0.3f * c) + 0.02f * y;
      }
  return x;
}

// what holds for every pair by the definition
static int invariants(const Out& o, const Out& swapped, int F) {
  const int D = max_disp(F);
  const size_t P = (size_t)o.H * o.W, nb = (size_t)o.side * o.side;
  int bad = !o.ok || !swapped.ok;
  for (int jd = 0; !bad && jd < o.nout * 2; ++jd) {
    const int64_t* sc = o.scal.data() + (size_t)jd * DG_DEFORM_SCALARS;
    int64_t total = 0;
    for (size_t i = 0; i < nb; ++i) { total += o.disp[jd * nb + i]; bad += o.disp[jd * nb + i] < 0; }
    bad += total != sc[0] || sc[1] < sc[0] || sc[1] > (int64_t)P || sc[4] < sc[0] || sc[4] > 65025 * sc[0] || sc[2] < 0 || sc[3] < 0;
    // the other call's other direction is this direction
    const int other = jd ^ 1;
    for (size_t i = 0; i < nb; ++i) bad += swapped.disp[other * nb + i] != o.disp[jd * nb + i];
    for (int e = 0; e < DG_DEFORM_SCALARS; ++e) bad += swapped.scal[(size_t)other * DG_DEFORM_SCALARS + e] != sc[e];
    // the morphed field is the source (the other side's morphed field under a zero displacement is not available here, so use
    // the bound only) and every vector stays within D
    for (size_t p = 0; p < P; ++p) {
      const int dy = o.field[((size_t)jd * 2 + 0) * P + p], dx = o.field[((size_t)jd * 2 + 1) * P + p];
      bad += dy < -D || dy > D || dx < -D || dx > D;
      bad += swapped.field[((size_t)other * 2 + 0) * P + p] != dy || swapped.field[((size_t)other * 2 + 1) * P + p] != dx;
      bad += swapped.mor[(size_t)other * P + p] != o.mor[(size_t)jd * P + p];
    }
  }
  return bad;
}

static int pair_case(int C, bool speed, int H, int W, int F, int sy, int sx) {
  const dg_deform_spec s = spec_of(C, speed, F);
  const std::vector<float> a = pattern(C, H, W, 0, 0), b = pattern(C, H, W, sy, sx);
  const Out o = run(s, C, a, b, H, W), sw = run(s, C, b, a, H, W), same = run(s, C, a, a, H, W);
  int bad = invariants(o, sw, F) + !same.ok;
  const int D = max_disp(F);
  const size_t P = (size_t)H * W, nb = (size_t)o.side * o.side;
  for (int jd = 0; !bad && jd < same.nout * 2; ++jd) {                  // identical fields: d = 0, no error, M = the field itself
    const int64_t* sc = same.scal.data() + (size_t)jd * DG_DEFORM_SCALARS;
    bad += sc[2] != 0 || sc[3] != 0 || sc[0] != sc[1] || same.disp[jd * nb + (size_t)D * same.side + D] != sc[0];
    for (size_t p = 0; p < 2 * P; ++p) bad += same.field[(size_t)jd * 2 * P + p] != 0;
    for (size_t p = 0; p < P; ++p) bad += same.mor[(size_t)jd * P + p] != same.mor[(size_t)(jd ^ 1) * P + p];
  }
  // the morphed field of the pair is the quantised source (known from the identical pair: M = q there) read through d_0
  const Out qb = run(s, C, b, b, H, W);
  for (int j = 0; !bad && j < o.nout; ++j)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w) {
        const size_t p = (size_t)h * W + w, jd = (size_t)j * 2;
        const int y = h + o.field[(jd * 2 + 0) * P + p], x = w + o.field[(jd * 2 + 1) * P + p];
        const int want = y >= 0 && y < H && x >= 0 && x < W ? qb.mor[jd * P + (size_t)y * W + x] : 0;
        bad += o.mor[jd * P + p] != want;
      }
  return report(speed ? "pattern pair, channels + speed" : "pattern pair", H, W, F, bad);
}

// two empty fields, a NaN field, and a saturated one: nothing moves
static int constant(int H, int W, int F, float fill) {
  const dg_deform_spec s = spec_of(1, false, F);
  const std::vector<float> a((size_t)H * W, fill);
  const Out o = run(s, 1, a, a, H, W);
  const bool on = fill == fill && fill >= 0.25f;
  const int64_t P = (int64_t)H * W, D = max_disp(F);
  int bad = !o.ok;
  for (int d = 0; !bad && d < 2; ++d) {
    const int64_t* sc = o.scal.data() + d * DG_DEFORM_SCALARS;
    bad += sc[0] != (on ? P : 0) || sc[1] != sc[0] || sc[2] != 0 || sc[3] != 0 || sc[4] != (on ? 65025 * P : 0);
    bad += o.disp[(size_t)d * o.side * o.side + D * o.side + D] != sc[0];
  }
  for (int16_t v : o.field) bad += v != 0;
  for (uint8_t v : o.mor) bad += v != (on ? 255 : 0);
  bad += dg_deform_bound(H, W) != 65025 * P;
  return report(fill != fill ? "NaN fields" : on ? "saturated fields" : "empty fields", H, W, F, bad);
}

// a bump moved by (sy, sx) well inside the grid: that vector is the most frequent one in both directions, and morphing lowers the error
static int found(int H, int W, int F, int sy, int sx) {
  const dg_deform_spec s = spec_of(1, false, F);
  std::vector<float> a((size_t)H * W), b((size_t)H * W);
  for (int h = 0; h < H; ++h)
    for (int w = 0; w < W; ++w) {
      const float ya = (float)(h - H / 2), xa = (float)(w - W / 2), yb = ya - sy, xb = xa - sx;
      a[(size_t)h * W + w] = 4.f * std::exp(-(ya * ya + xa * xa) / 50.f);
      b[(size_t)h * W + w] = 4.f * std::exp(-(yb * yb + xb * xb) / 50.f);
    }
  const Out o = run(s, 1, a, b, H, W);
  const int D = max_disp(F);
  int bad = !o.ok;
  if (!bad) {
    const size_t nb = (size_t)o.side * o.side;
    const int64_t hit = o.disp[(size_t)(sy + D) * o.side + sx + D], back = o.disp[nb + (size_t)(-sy + D) * o.side + -sx + D];
    for (size_t i = 0; i < nb; ++i) bad += o.disp[i] > hit || o.disp[nb + i] > back;     // the modal vector is the move
    bad += hit <= 0 || back <= 0 || o.scal[2] >= o.scal[3] || o.scal[DG_DEFORM_SCALARS + 2] >= o.scal[DG_DEFORM_SCALARS + 3];
  }
  return report("moved bump", H, W, F, bad);
}

int main() {
  int bad = 0;
  const int grids[][2] = {{1, 1}, {1, 70}, {70, 1}, {5, 3}, {17, 33}, {37, 53}};
  for (const auto& g : grids)
    for (int F = 1; F <= DG_DEFORM_MAX_LEVELS; ++F) {
      bad += pair_case(1, false, g[0], g[1], F, 2, -3);
      bad += constant(g[0], g[1], F, 0.f) + constant(g[0], g[1], F, NAN) + constant(g[0], g[1], F, 1e9f);
    }
  bad += pair_case(2, true, 19, 22, 2, 1, 4) + pair_case(DG_EOF_MAX_C, true, 9, 14, 3, -2, 1) + pair_case(3, false, 12, 7, 4, 3, 3);
  bad += found(40, 48, 1, 2, -3) + found(40, 48, 2, -5, 4) + found(48, 56, 3, 7, 6);
  // rejected arguments return a status and touch nothing
  const dg_deform_spec s = spec_of(1, false, 1);
  dg_deform_spec none = s, step = s, lo = s;
  none.levels = 0;
  step.inv_step[0] = 0.f;
  lo.lo[0] = INFINITY;
  std::vector<float> x(4, 0.f);
  std::vector<int64_t> disp(2 * 13 * 13, 0), scal(2 * DG_DEFORM_SCALARS, 0);
  std::vector<int16_t> field(2 * 2 * 4, 0);
  bad += dg_deform_host(&none, x.data(), x.data(), 1, 2, 2, disp.data(), scal.data()) == DG_OK;
  bad += dg_deform_host(&step, x.data(), x.data(), 1, 2, 2, disp.data(), scal.data()) == DG_OK;
  bad += dg_deform_host(&lo, x.data(), x.data(), 1, 2, 2, disp.data(), scal.data()) == DG_OK;
  bad += dg_deform_host(&s, x.data(), x.data(), 1, 0, 2, disp.data(), scal.data()) == DG_OK;
  bad += dg_deform_host(&s, x.data(), x.data(), 1, 2, 2049, disp.data(), scal.data()) == DG_OK;
  bad += dg_deform_host(&s, nullptr, x.data(), 1, 2, 2, disp.data(), scal.data()) == DG_OK;
  bad += dg_deform_host(&s, x.data(), x.data(), 1, 2, 2, nullptr, scal.data()) == DG_OK;
  bad += dg_deform_field_host(&s, x.data(), x.data(), 1, 2, 2, nullptr, nullptr) == DG_OK;
  bad += dg_deform_field_host(&s, x.data(), x.data(), 1, 2, 2, field.data(), nullptr) != DG_OK;      // morphed is optional
  bad += dg_deform_bound(0, 1) != 0 || dg_deform_bound(2049, 1) != 0;
  for (int64_t v : disp) bad += v != 0;
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
