// Weight-stationary streaming kernel for the data gradient of a 3x3, stride-2, pad-1 conv with 128 -> 128 channels in bf16
// (the critic's features.2: dx is 8.6 GB at batch 32, the whole reduction 128 channels).
//
// The tile kernel (conv_halo.hip, SEG) streams the weights and keeps a pixel tile: at this layer a 64-KB output tile has 2-8
// tap-steps of MFMA work and pays a patch prologue, a weight DMA per step and a store-burst epilogue around them.  Here the roles
// are swapped: all nine taps (288 KiB) live in the registers of ONE 8-wave workgroup per CU for the whole launch, and dy streams
// through.  The workgroup walks a column strip of dy (16 pixels wide) top to bottom; step r reads dy rows r and r + 1 (17 pixels
// each: the strip and its right neighbour) from a three-slot LDS ring and writes the two dx rows 2r and 2r + 1 of the strip
// (32 pixels each).  Row r + 2 and the 1 KB of mask words of step r + 1, fetched to registers a step earlier, are written to the
// third slot at the end of the step: one barrier per step, no per-tile prologue or epilogue.
//
// Wave w owns the 32 dx channels of quarter w & 3.  Waves 0-3 hold the four taps of parity class (1,1) (32 A fragments = 128
// registers), waves 4-7 the five taps of classes (0,0), (0,1) and (1,0) (40 fragments = 160 registers): every SIMD hosts one wave
// of each kind, 32 + 40 MFMAs per step.  Every accumulation chain is local to one wave and runs in the tile kernel's order
// (reduction block, then the class's taps in planner order, then k-block 0, 1; accumulators start at zero; the same conversion
// and mask multiply), so the result is bit-identical to the SEG launch.
//
// A fragment row m of channel fragment j is dx channel 32q + 8(m >> 2) + 4j + (m & 3): lane group g then holds the eight
// consecutive channels 32q + 8g .. + 7 of its pixel -- one 16-byte store per lane and class, 64-byte runs per pixel and wave.
// (Staging the two dx rows of a step through LDS and storing contiguous 1-KB runs per wave measured no faster: profiles/NOTES.md.)
#include "gg_common.h"

namespace {

constexpr int NT = 512;                  // 8 waves
constexpr int RING_PIX = 17;             // 16 dy pixels of the strip + the right neighbour
// 256 B of channels + 32 B: lane (l15, g) of a ds_read_b128 sits in 16-byte slot (2 * l15 + g) mod 16 of the 256-byte bank row,
// distinct for the 16 lanes the LDS serves per cycle
constexpr int RING_PITCH = 288;
constexpr int MASK_OFF = RING_PIX * RING_PITCH;   // behind the dy row of a slot: the mask words of the step that reads it as row r + 1
constexpr int RING_ROW = MASK_OFF + 2 * 32 * 16;  // ... two dx rows x 32 pixels x 16 bytes
constexpr int RING_CHUNKS = RING_PIX * 16;   // 16-byte pieces of one ring row

struct S2DArgs {
  const char* dy; const char* w; char* dx; const char* mask_bits;
  float slope;
  int Ho, Wo;                 // dy grid; dx is 2Ho x 2Wo
  int nstrips, nitems, trips; // strips per image, (image, strip) items, items per workgroup (the last may fall outside)
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const char* p) {
  const unsigned long long b = (unsigned long long)p;
  const unsigned long long u = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32)) << 32) |
                               (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  return __builtin_amdgcn_make_buffer_rsrc((void*)u, 0, (int)DG_OOB_OFF, 0x00020000);
}

// the lane's eight channels of one pixel: LeakyReLU' from the mask byte, bf16, one 16-byte store
template <bool MASK>
__device__ __forceinline__ void store_pixel(const f32x4_t& f0, const f32x4_t& f1, unsigned mb, float slope, __amdgpu_buffer_rsrc_t rY,
                                            unsigned off) {
  float v[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
  if (MASK) {
    // v *= bit ? 1 : slope, as the tile kernel's epilogue.  The byte's bits leave through the carry, from the top: one add puts bit e
    // into VCC and moves bit e - 1 up, one select picks the factor -- two operations per value where and / compare / select take three
    // (this epilogue runs beside the MFMAs of the SIMD's other wave and is bound by instruction issue)
    unsigned sh = mb << 24;
    const float one = 1.f;
#pragma unroll
    for (int e = 7; e >= 0; --e) {
      float f;
      asm("v_add_co_u32_e32 %1, vcc, %1, %1\n\tv_cndmask_b32_e32 %0, %2, %3, vcc" : "=&v"(f), "+v"(sh) : "v"(slope), "v"(one) : "vcc");
      v[e] *= f;
    }
  }
  u32x4_t t;
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = pack_bf16x2(v[2 * k], v[2 * k + 1]);
  __builtin_amdgcn_raw_buffer_store_b128(t, rY, off, 0, 0);
}

// C11: waves 0-3 (class (1,1), taps w0 w2 w6 w8), else waves 4-7 (classes (0,0): w4; (0,1): w3 w5; (1,0): w1 w7)
template <bool MASK, bool C11>
__device__ __forceinline__ void s2d_run(const S2DArgs& a, char* ring) {
  constexpr int NTAP = C11 ? 4 : 5;
  const int tid = threadIdx.x, lane = tid & 63, q = (tid >> 6) & 3;
  const int l15 = lane & 15, g = lane >> 4;

  // stationary weights: wr[((cb * NTAP + t) * 2 + kk) * 2 + j], A fragment row l15 = dx channel `n`, K = channels 64cb + 32kk + 8g .. + 7
  // of tap t of the data-gradient pack [dx channel][tap][dy channel]
  uint4 wr[NTAP * 8];
  {
    constexpr int TW11[4] = {0, 2, 6, 8}, TWX[5] = {4, 3, 5, 1, 7};
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int n = 32 * q + 8 * (l15 >> 2) + 4 * j + (l15 & 3);
            const int tw = C11 ? TW11[t] : TWX[t];
            wr[((cb * NTAP + t) * 2 + kk) * 2 + j] =
                *reinterpret_cast<const uint4*>(a.w + ((long long)n * 1152 + tw * 128 + 64 * cb + 32 * kk + 8 * g) * 2);
          }
  }

  const int W = 2 * a.Wo;
  // B fragment of shift sx: pixel l15 + sx of a ring row, channels 64cb + 32kk + 8g .. + 7
  const char* const fb0 = ring + l15 * RING_PITCH + g * 16;
  const int fill_pix = tid >> 4;                                        // this thread's 16-byte piece of a ring row (tid < RING_CHUNKS)
  char* const fill_dst = ring + fill_pix * RING_PITCH + (tid & 15) * 16;
  const bool filler = tid < RING_CHUNKS;

  for (int trip = 0; trip < a.trips; ++trip) {
    const int item = (int)blockIdx.x + trip * (int)gridDim.x;           // workgroup-uniform
    if (item >= a.nitems) break;
    const int img = item / a.nstrips, x0 = (item - img * a.nstrips) * 16;
    const __amdgpu_buffer_rsrc_t rX = uniform_rsrc(a.dy + ((long long)img * a.Ho * a.Wo + x0) * 256);
    const __amdgpu_buffer_rsrc_t rY = uniform_rsrc(a.dx + ((long long)img * 2 * a.Ho * W + 2 * x0) * 256);
    const __amdgpu_buffer_rsrc_t rM = uniform_rsrc(MASK ? a.mask_bits + ((long long)img * 2 * a.Ho * W + 2 * x0) * 16 : a.dx);
    // out-of-range pieces (columns past the image; rows past it below) read as zero, out-of-range pixels are not stored
    const unsigned fill_off = (filler && x0 + fill_pix < a.Wo) ? (unsigned)tid * 16u : DG_OOB_OFF;
    const unsigned pix_ok = x0 + l15 < a.Wo ? 0u : DG_OOB_OFF;
    const unsigned st_lane = pix_ok | (unsigned)(2 * l15 * 256 + 64 * q + 16 * g);        // class column parity adds 256
    auto fetch_row = [&](int rr) {
      // (fill_off + row offset < 2^32: an out-of-range piece stays out of range)
      return __builtin_amdgcn_raw_buffer_load_b128(rX, rr < a.Ho ? fill_off + (unsigned)rr * (unsigned)a.Wo * 256u : DG_OOB_OFF, 0, 0);
    };
    // The mask words of a step (two dx rows x 32 pixels x 16 bytes = one 16-byte piece per lane of wave 5) travel with the dy row
    // that enters the ring for that step: one load per step and workgroup instead of a byte load per lane and class, fetched two
    // steps ahead like the row.  A lane then reads its byte (channels 32q + 8g .. + 7) from the slot of row r + 1.
    const bool mwave = MASK && !C11 && __builtin_amdgcn_readfirstlane(tid >> 6) == 5;
    const int ml = tid & 63;                                            // (row parity, pixel) = (ml >> 5, ml & 31)
    const unsigned mfill_off = 2 * x0 + (ml & 31) < W ? (unsigned)(((ml >> 5) * W + (ml & 31)) * 16) : DG_OOB_OFF;
    char* const mfill_dst = ring + MASK_OFF + ml * 16;
    auto fetch_mask = [&](int k) {                                      // of step k
      return __builtin_amdgcn_raw_buffer_load_b128(rM, k < a.Ho ? mfill_off + (unsigned)(2 * k) * (unsigned)W * 16u : DG_OOB_OFF, 0, 0);
    };
    const char* const mrd = ring + MASK_OFF + 2 * l15 * 16 + 4 * q + g;  // class (ph, pw) at + 512 ph + 16 pw
    // rows 0 and 1 with step 0's masks (every wave is past the previous item's last step: its closing barrier); row 2 and step 1's
    // masks are staged
    {
      const u32x4_t r0 = fetch_row(0), r1 = fetch_row(1);
      if (filler) {
        *reinterpret_cast<uint4*>(fill_dst) = __builtin_bit_cast(uint4, r0);
        *reinterpret_cast<uint4*>(fill_dst + RING_ROW) = __builtin_bit_cast(uint4, r1);
      }
      if (mwave) *reinterpret_cast<uint4*>(mfill_dst + RING_ROW) = __builtin_bit_cast(uint4, fetch_mask(0));
    }
    u32x4_t st0 = fetch_row(2), st1;
    u32x4_t ms0 = {0u, 0u, 0u, 0u}, ms1 = {0u, 0u, 0u, 0u};
    if (mwave) ms0 = fetch_mask(1);
    __syncthreads();
    int sA = 0, sB = RING_ROW, sC = 2 * RING_ROW;                       // ring slots of rows r, r + 1, r + 2
    // One step.  dy row r + 3 and the masks of step r + 2 are fetched now; row r + 2 and the masks of step r + 1 -- `staged`, `mstaged`,
    // fetched a step ago -- go to the ring at the end of this step.  The loop below alternates two register sets, so nothing staged
    // is copied (a copy waits for its load).
    auto step = [&](int r, const u32x4_t& staged, u32x4_t& nxt, const u32x4_t& mstaged, u32x4_t& mnxt) __attribute__((always_inline)) {
      nxt = fetch_row(r + 3);
      if (mwave) mnxt = fetch_mask(r + 2);
      unsigned mb[3] = {0u, 0u, 0u};
      if (MASK) {
        if (C11) {
          mb[0] = *reinterpret_cast<const unsigned char*>(mrd + sB + 512 + 16);
        } else {
          mb[0] = *reinterpret_cast<const unsigned char*>(mrd + sB);
          mb[1] = *reinterpret_cast<const unsigned char*>(mrd + sB + 16);
          mb[2] = *reinterpret_cast<const unsigned char*>(mrd + sB + 512);
        }
      }
      const unsigned row0 = (unsigned)(2 * r) * (unsigned)W;             // dx pixel offset of row 2r inside the strip's view
      __builtin_amdgcn_sched_barrier(0);
      auto frag = [&](int slot, int sx, int cb, int kk) {
        return *reinterpret_cast<const uint4*>(fb0 + slot + sx * RING_PITCH + cb * 128 + kk * 64);
      };
      if constexpr (C11) {
        f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int t = 0; t < 4; ++t)          // taps (dy, dx) = (1,1) (1,0) (0,1) (0,0)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
              const uint4 b = frag(t < 2 ? sB : sA, (t & 1) ? 0 : 1, cb, kk);
#pragma unroll
              for (int j = 0; j < 2; ++j) Mma<bf16_t>::run(wr[((cb * 4 + t) * 2 + kk) * 2 + j], b, acc[j]);
            }
        store_pixel<MASK>(acc[0], acc[1], mb[0], a.slope, rY, st_lane + (row0 + W + 1) * 256u);
      } else {
        // class by class, each store behind its chain: the conversion and store of one class issue between the MFMAs of the next
        auto tap = [&](int cb, int t, const uint4 (&b)[2], f32x4_t (&ac)[2]) {
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 2; ++j) Mma<bf16_t>::run(wr[((cb * 5 + t) * 2 + kk) * 2 + j], b[kk], ac[j]);
        };
        uint4 b00[2][2];                                 // shift (0,0): every class reads it
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) b00[cb][kk] = frag(sA, 0, cb, kk);
        {                                                // class (0,0): w4
          f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) tap(cb, 0, b00[cb], acc);
          store_pixel<MASK>(acc[0], acc[1], mb[0], a.slope, rY, st_lane + row0 * 256u);
        }
        {                                                // class (0,1): w3 at (0,1), w5 at (0,0)
          f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            const uint4 b01[2] = {frag(sA, 1, cb, 0), frag(sA, 1, cb, 1)};
            tap(cb, 1, b01, acc); tap(cb, 2, b00[cb], acc);
          }
          store_pixel<MASK>(acc[0], acc[1], mb[1], a.slope, rY, st_lane + (row0 + 1) * 256u);
        }
        {                                                // class (1,0): w1 at (1,0), w7 at (0,0)
          f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            const uint4 b10[2] = {frag(sB, 0, cb, 0), frag(sB, 0, cb, 1)};
            tap(cb, 3, b10, acc); tap(cb, 4, b00[cb], acc);
          }
          store_pixel<MASK>(acc[0], acc[1], mb[2], a.slope, rY, st_lane + (row0 + W) * 256u);
        }
      }
      if (filler) *reinterpret_cast<uint4*>(fill_dst + sC) = __builtin_bit_cast(uint4, staged);
      if (mwave) *reinterpret_cast<uint4*>(mfill_dst + sC) = __builtin_bit_cast(uint4, mstaged);
      __syncthreads();
      const int s = sA; sA = sB; sB = sC; sC = s;
    };
    for (int r = 0; r < a.Ho; r += 2) {
      step(r, st0, st1, ms0, ms1);
      if (r + 1 < a.Ho) step(r + 1, st1, st0, ms1, ms0);
    }
  }
}

std::atomic<int> g_s2_stream{1};
std::atomic<int> g_cus{0};

}  // namespace

// (outside the unnamed namespace: profilers then list the kernel under its own name)
template <bool MASK>
__global__ __launch_bounds__(NT, 1) void s2dgrad_stream_kernel(const S2DArgs a) {
  __shared__ __attribute__((aligned(16))) char ring[3 * RING_ROW];
  // both halves run the same trips, steps and barriers
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) < 4) s2d_run<MASK, true>(a, ring);
  else s2d_run<MASK, false>(a, ring);
}

// One host function decides: bf16, 128 -> 128 channels with dense pixels on both sides, stride 2, plain or mask_bits epilogue,
// rows the halo kernel's limit allows and images whose byte offsets fit the kernel's 32-bit lane offsets.
bool s2dgrad_stream_eligible(const dg_conv_geom* g, const dg_epilogue* ep) {
  if (!g || g->dtype != DG_BF16 || g->stride != 2 || g->pixel_shuffle) return false;
  if (g->N <= 0 || g->H <= 0 || g->W <= 0 || ((g->H | g->W) & 1)) return false;
  if (g->Cin != 128 || g->Cout != 128 || g->ldx != 128 || g->ldy != 128) return false;
  if (!gg_halo_row_step_ok(g->W / 2, g->ldy, g->dtype, 1)) return false;
  if ((long long)g->H * g->W * 256 >= (1ll << 31)) return false;
  if (ep && (ep->bias || ep->has_act || ep->r1 || ep->r2 || ep->mask || ep->accumulate || ep->out_bits || ep->mask_c0 || ep->mask_last ||
             ep->out_q || ep->out_qs || ep->out_u || ep->out_ue || ep->skip_y || ep->out_amax))
    return false;
  return true;
}

int s2dgrad_stream_mode() { return g_s2_stream.load(std::memory_order_relaxed); }

extern "C" int dg_set_s2_dgrad_stream(int on) { return g_s2_stream.exchange(on < 0 ? 0 : on, std::memory_order_relaxed); }

int s2dgrad_stream_launch(const dg_conv_geom* g, const dg_epilogue* ep, const void* dy, const void* w, void* dx, hipStream_t st) {
  if (!dy || !w || !dx) return DG_ERR_BAD_ARG;
  int cus = g_cus.load(std::memory_order_relaxed);
  if (cus <= 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return DG_ERR_LAUNCH;
    g_cus.store(cus, std::memory_order_relaxed);
  }
  S2DArgs a{};
  a.dy = (const char*)dy; a.w = (const char*)w; a.dx = (char*)dx;
  a.mask_bits = ep ? (const char*)ep->mask_bits : nullptr;
  a.slope = ep ? ep->mask_slope : 1.f;
  a.Ho = g->H / 2; a.Wo = g->W / 2;
  a.nstrips = (a.Wo + 15) / 16;
  const long long items = (long long)g->N * a.nstrips;
  if (items >= (1ll << 31)) return DG_ERR_BAD_SHAPE;
  a.nitems = (int)items;
  // one workgroup per CU (a switch value n > 1 caps the grid at n workgroups: tests walk the persistent loop at small shapes)
  const int mode = s2dgrad_stream_mode();
  int grid = mode > 1 && mode < cus ? mode : cus;
  if (grid > a.nitems) grid = a.nitems;
  a.trips = (a.nitems + grid - 1) / grid;
  g_last_kinds |= 64;
  if (a.mask_bits) hipLaunchKernelGGL(s2dgrad_stream_kernel<true>, dim3(grid), dim3(NT), 0, st, a);
  else hipLaunchKernelGGL(s2dgrad_stream_kernel<false>, dim3(grid), dim3(NT), 0, st, a);
  return dg_check_launch();
}
