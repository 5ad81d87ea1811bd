/*
 * downgan_hip.h — C ABI of libdowngan_hip.so: the MI355X (gfx950) kernels of the DoWnGAN WGAN-GP
 * train step.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * The reference (nannau/DoWnGAN) has no FFI of its own: its hot path is PyTorch ops called from
 * DoWnGAN/GAN/wasserstein.py and DoWnGAN/networks/{generator,critic}.py.  Each entry point below
 * names the reference op / call site it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - Activations are NHWC ("channels-last"), element type `dtype` (DG_F32 or DG_BF16), channel
 *    counts padded to a multiple of 16, `ld*` = distance between consecutive pixels in ELEMENTS
 *    (so a tensor may be a channel slice of a wider dense-block slab).  All base pointers and
 *    channel offsets are 16-byte aligned.
 *  - Conv weights are packed [Nout][9 taps][Cred] in `dtype` (see dg_repack_conv_weights): the
 *    forward pack has Nout=Cout, Cred=Cin (KRSC); the dgrad pack has Nout=Cin, Cred=Cout.
 *  - Master parameters, gradients, Adam moments, biases and all loss scalars are fp32.
 *  - Ownership: the caller owns every buffer (incl. workspaces); nothing here allocates or frees
 *    device memory.  Launches are asynchronous on `stream` (a hipStream_t passed as void*).
 *  - Errors: 0 = DG_OK, negative = dg_status; no exceptions cross the ABI.
 *  - Re-entrant.  The only mutable state is a per-kernel, per-device "function attributes configured" mask
 *    (hipFuncAttributeMaxDynamicSharedMemorySize is set once per device) and cached occupancy answers, both
 *    std::atomic; the device that is current when an entry point is called must be the device of `stream`.
 */
#ifndef DOWNGAN_HIP_H
#define DOWNGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_F32 0
#define DG_BF16 1

typedef enum dg_status {
  DG_OK = 0,
  DG_ERR_BAD_SHAPE = -1,
  DG_ERR_BAD_DTYPE = -2,
  DG_ERR_BAD_ARG = -3,
  DG_ERR_LAUNCH = -4
} dg_status;

/* Epilogue applied to every output element v (fp32 accumulator) before the store, in this order:
 *   v += bias[c]; if (has_act) v = v>0 ? v : v*act_slope;
 *   if (r1) v = v*s1 + r1[pixel,c];  if (r2) v = v*s2 + r2[pixel,c];
 *   if (mask) v *= (mask[pixel,c] > 0 ? 1 : mask_slope);     -- LeakyReLU'(saved activation)
 *   if (accumulate) v += y[pixel,c];
 * r1/r2/mask are tensors of the OUTPUT's shape in `dtype`.
 * mask_c0 / mask_last (both 0 = the order above, every channel): the mask applies to channels c >= mask_c0 only
 * (multiple of 16), and with mask_last != 0 it multiplies AFTER the accumulate -- the data gradient of a dense block's
 * conv k completes channel slice k-1 of the block's gradient slab and applies that slice's LeakyReLU' in the same pass.
 * mask_c0 != 0 is refused (DG_ERR_BAD_SHAPE) for a pixel-shuffled destination, whose channels are not the GEMM's columns. */
typedef struct dg_epilogue {
  const float* bias;
  int has_act;
  float act_slope;
  const void* r1; int64_t ldr1; float s1;
  const void* r2; int64_t ldr2; float s2;
  const void* mask; int64_t ldmask; float mask_slope;
  int accumulate;
  /* 1-bit form of the LeakyReLU' mask (16x fewer bytes than re-reading the activation; the critic's data-gradient
   * epilogues are HBM-bound on it): a tensor [pixel][Cout/64][4] of uint16, bit b of word (block, g) belonging to channel
   * 64*block + 16g + b -- a little-endian bit string over the channels of a pixel.  mask_bits: multiply by (bit ? 1 : mask_slope) (instead of `mask`); out_bits: written by this
   * launch as (stored value > 0).  Both need Cout % 64 == 0, Cout >= 128 and no pixel shuffle. */
  const void* mask_bits;
  void* out_bits;
  int mask_c0;
  int mask_last;
  /* MXFP8 copy of the stored output for the fp8 conv path (see dg_quant_mxfp8 below): out_q [pixel][ld of y] E4M3 bytes
   * (same pixel stride as y, counted in bytes) and out_qs [pixel][Cout/32] E8M0 scale bytes, bit-identical to
   * dg_quant_mxfp8 of the bf16 tensor this launch stores -- the next layer's fp8 conv reads them instead of a separate
   * quantisation pass.  Both or neither; bf16 launches with Cout % 64 == 0, Cout >= 128, no pixel shuffle.
   * ldqs: scale bytes per pixel of out_qs (0 = Cout/32, dense); a larger stride addresses a channel slice of a wider tensor
   * (dense-block slab: y, out_q and out_qs all point at the slice's first channel) and needs Cout/16 to be a power of two. */
  void* out_q;
  void* out_qs;
  int64_t ldqs;
  /* Second fp8 copy of the stored output for the fp8 WEIGHT GRADIENT (dg_conv3x3_wgrad_f8), whose contraction runs over pixels:
   * out_u [pixel][ld of y] E4M3 bytes = stored value / 2^(out_ue[channel / 32] - 127), saturated at +-448, with ONE exponent
   * byte per 32-channel block for the whole tensor (out_ue: Cout / 32 bytes of device memory, read by the launch; the caller
   * derives them from an earlier pass, dg_block_exp_max).  Needs out_q (the copy is formed from the same rounded values). */
  void* out_u;
  const void* out_ue;
  /* != 0: the output tensor y itself is NOT stored -- only its fp8 copies (out_q or out_u required) / mask bits are, for launches whose
   * bf16 result nobody reads (fp8 mode: the next conv reads out_q, the weight gradient out_u, the masks out_bits).  Not with accumulate. */
  int skip_y;
  /* First-layer launches (<= 2 real input channels, critic.py:21-24: an 8.6-GB output at configs[1], store-bound) may write out_u
   * WITHOUT out_q -- the next layer's MXFP8 conv then reads the uniform-scale copy with out_ue as ONE scale row for every pixel
   * (dg_f8_operands.ldxs < 0): half the bytes -- and keep the census the exponents of the next pass come from themselves:
   * out_amax [Cout / 32] uint32 (device, zeroed by the caller / by dg_exp_from_amax), atomically maxed with the bit pattern of the
   * largest |stored value| of each 32-channel block.  Other launches return DG_ERR_BAD_SHAPE for either. */
  void* out_amax;
} dg_epilogue;

/* Geometry of ONE reference nn.Conv2d(Cin, Cout, kernel_size=3, stride, padding=1) layer
 * (generator.py:24,62,66,70,77,80; critic.py:21-87), in its FORWARD orientation. */
typedef struct dg_conv_geom {
  int dtype;
  int N, H, W;          /* forward input: N images of H x W                                     */
  int Cin, Cout;        /* padded channel counts (multiples of 16; Cin may be a multiple of 8)   */
  int stride;           /* 1 or 2; output is Ho = H/stride, Wo = W/stride (H, W even if 2)       */
  int cin_real;         /* number of REAL (non-padding) input channels, 0 = unknown/all. Layers   */
                        /*    with <= 2 real channels (critic features.0, critic.py:21) take an    */
                        /*    im2col path that reads the big tensor once for all 9 taps.           */
  int pixel_shuffle;    /* 1: the layer is followed by LeakyReLU + nn.PixelShuffle(2)            */
                        /*    (generator.py:69-75). Output channels are packed (2i+j)*Cout/4 + c */
                        /*    and the activation tensor is stored shuffled: [N,2Ho,2Wo,Cout/4].  */
  int64_t ldx;          /* pixel stride of the layer INPUT tensor x  (or of dx in dgrad)         */
  int64_t ldy;          /* pixel stride of the layer OUTPUT tensor y (or of dy in dgrad/wgrad)   */
} dg_conv_geom;

/* The generic launch descriptor every conv forward / data-gradient is lowered to: a gather-GEMM
 *   Y[dst(m), n] = epilogue( sum_{t<ntaps} sum_{c<Cred} X[src(m,t), c] * Wp[n][tap_w[t]][c] )
 * over GEMM rows m = (img, gy, gx) of an Hg x Wg grid, src(m,t) = (img, gy*sy_mul+tap_dy[t],
 * gx*sx_mul+tap_dx[t]) (zero outside the source), dst(m) = (img, gy*dy_mul+dy_off, gx*dx_mul+dx_off).
 * Exposed so that the planner can be checked on a CPU (dg_conv3x3_plan needs no GPU). */
typedef struct dg_gg_desc {
  int dtype;
  int N, Hs, Ws, Cred; int64_t lds;   /* source tensor                                          */
  int src_ps;                          /* source is stored pixel-shuffled (Cred = 4*Cps)         */
  int Hg, Wg, sy_mul, sx_mul;
  int ntaps; int tap_dy[9], tap_dx[9], tap_w[9];
  int Nout; int64_t ldw;               /* packed weights: row stride in elements (9*Cred)        */
  int Hd, Wd; int64_t ldd;             /* destination tensor                                     */
  int dy_mul, dx_mul, dy_off, dx_off;
  int dst_ps;                          /* store pixel-shuffled (Nout = 4*Cps)                    */
} dg_gg_desc;

const char* dg_version(void);

/* ---- convolution family (replaces torch.nn.Conv2d forward/backward on the hot path) ---------- */

/* y = epilogue(conv3x3(x, w_fwd)).  Replaces nn.Conv2d.forward (+ fused LeakyReLU / residual /
 * PixelShuffle): generator.py:36-41,53,62-90; critic.py:101-102. */
int dg_conv3x3_fwd(const dg_conv_geom* g, const dg_epilogue* ep, const void* x, const void* w_fwd,
                   void* y, void* stream);

/* dx = epilogue(conv3x3_input_grad(dy, w_dgrad)).  Replaces the autograd input-gradient of
 * nn.Conv2d (wasserstein.py:52,80 backward; :100-106 autograd.grad for the penalty).  Stride 2 is
 * done as 4 output-parity classes (no zero insertion).  Epilogue tensors have dx's shape. */
int dg_conv3x3_dgrad(const dg_conv_geom* g, const dg_epilogue* ep, const void* dy,
                     const void* w_dgrad, void* dx, void* stream);

/* dw[Cout][9][Cin] (fp32) += sum_pixels dy (x) x   (atomic accumulate).  Replaces the autograd
 * weight-gradient of nn.Conv2d (wasserstein.py:52,80) and, with (x:=tangent, dy:=adjoint), the
 * double-backward term of the gradient penalty (wasserstein.py:100-117 under :52). */
int dg_conv3x3_wgrad(const dg_conv_geom* g, const void* x, const void* dy, float* dw, float* db,
                     void* stream);
  /* db (optional): bias gradient += sum_pixels dy */

/* Weight and bias gradients of ALL convs of a dense block (generator.py:14-41) in one launch.  Conv k = 1..nconv reads channels
 * [0, k*128) of the block's activation slab x [N,H,W,nconv*128] and its output adjoint is channels [(k-1)*128, k*128) of the
 * adjoint slab dy; dw[k-1] ([128][9][k*128] fp32) and db[k-1] ([128] fp32, db or any entry may be NULL) are accumulated into.
 * g: Cin = Cout = nconv*128, stride 1, ldx / ldy = pixel strides of the two slabs; bf16; W % 32 == 0. */
int dg_conv3x3_wgrad_dense(const dg_conv_geom* g, int nconv, const void* x, const void* dy,
                           float* const* dw, float* const* db, void* stream);

/* fp8 weight gradient (BASELINE.json configs[4]; autograd of DoWnGAN/networks/critic.py:34-88 under GAN/wasserstein.py:52):
 * dw[co][tap][ci] (fp32, accumulated into) += sum_p dy[p, co] * x[src(p, tap), ci] with E4M3 operands whose scale does not vary
 * along pixels -- the contraction index -- : x = xq * 2^(ex[ci / 32] - 127), dy = dyq * 2^(ey[co / 32] - 127), one E8M0 exponent
 * byte per 32-channel block of the whole tensor (device arrays of Cin / 32 and Cout / 32 bytes).  g->ldx / g->ldy are the pixel
 * strides of xq / dyq in bytes (= elements, multiples of 16); g->dtype = DG_BF16 (the precision the fp8 forms stand for).  Stride 1
 * or 2, Cin and Cout multiples of 128, OUTPUT rows (W / stride) a multiple of 64 pixels, no pixel shuffle; anything else returns
 * DG_ERR_BAD_SHAPE (callers keep the bf16 kernel). */
int dg_conv3x3_wgrad_f8(const dg_conv_geom* g, const void* xq, const void* ex, const void* dyq, const void* ey, float* dw,
                        void* stream);

/* dg_conv3x3_wgrad_dense on the fp8 kernel (autograd of DoWnGAN/networks/generator.py:24-41 under GAN/wasserstein.py:80 in fp8 mode):
 * xq / dyq = uniform-scale E4M3 copies of the block's activation and adjoint slabs [N,H,W,nconv*128] (pixel strides g->ldx / g->ldy
 * in bytes), ex / ey = their nconv*4 block exponents (as dg_conv3x3_wgrad_f8); dw[k-1] ([128][9][k*128] fp32) accumulated into.
 * Weight gradients only: the bias gradients are column sums of the adjoint slab (dg_colsum).  Stride 1, W a multiple of 64. */
int dg_conv3x3_wgrad_dense_f8(const dg_conv_geom* g, int nconv, const void* xq, const void* ex, const void* dyq, const void* ey,
                              float* const* dw, void* stream);

/* db[c] (fp32) += sum over rows of dy[row, c]  (bias gradient of a conv or Linear).  Row r is at
 * element offset (r / rows_inner)*ld_outer + (r % rows_inner)*ld, so one sub-position of a
 * pixel-shuffled tensor can be reduced (rows_outer x rows_inner rows in total). */
int dg_colsum(int dtype, const void* dy, int64_t rows_outer, int64_t ld_outer, int64_t rows_inner,
              int64_t ld, int C, float* db, void* stream);

/* One pass over a wide tensor, nseg (<= 8) destinations: db[k][c] (fp32) += sum over rows of dy[row, k*(C/nseg) + c]; rows of `ld`
 * elements.  The five bias gradients of a dense block (generator.py:24-41) from its adjoint slab when the weight gradients run on
 * dg_conv3x3_wgrad_dense_f8 (the bf16 dense launch sums them itself). */
int dg_colsum_multi(int dtype, const void* dy, int64_t rows, int64_t ld, int C, int nseg, float* const* db, void* stream);

/* Launches one gather-GEMM descriptor (what dg_conv3x3_fwd / _dgrad call after planning). */
int dg_gather_gemm(const dg_gg_desc* d, const dg_epilogue* ep, const void* x, const void* w, void* y,
                   void* stream);

/* Which kernel variants the calling thread's last dg_conv3x3_fwd / _dgrad launched (bit mask: 1 generic
 * gather-GEMM, 2 fast path, 8 halo-patch kernel, 16 im2col small-Cin kernel, 32 fp8 halo kernel, 64 streaming stride-2
 * data-gradient kernel). Diagnostic. */
int dg_last_conv_kernels(void);

/* Which launcher served the calling thread's last dg_conv3x3_wgrad / _wgrad_dense / _wgrad_f8 / _wgrad_dense_f8 call: 0 none (the
 * call returned before a launch), 1 per-tap kernel, 2 im2col kernel (<= 2 real input channels), 3 narrow row-of-taps kernel,
 * 4 wide row-of-taps kernel at stride 1, 5 wide kernel at stride 2, 6 dense-block launch of the wide kernel, 7 fp8 kernel.
 * Reset at the entry of each of those calls.  Diagnostic. */
int dg_last_wgrad_kernel(void);

/* Host-only planner (no GPU needed): lowers a layer to its gather-GEMM descriptor(s).
 * kind 0 = forward (1 desc), kind 1 = dgrad (1 desc for stride 1, 4 parity classes for stride 2).
 * Returns the number of descriptors written to out[0..3], or a negative dg_status. */
int dg_conv3x3_plan(const dg_conv_geom* g, int kind, dg_gg_desc* out);

/* Host-only: how dg_conv3x3_dgrad launches geometry g -- 1 = the four parity classes of a stride-2 layer merged into one launch
 * of the halo kernel (or a stride-1 layer's single class), 4 = one launch per class (narrow layers, or rows too long for the halo
 * kernel's 24-bit row step), negative = dg_status. */
int dg_conv3x3_dgrad_launches(const dg_conv_geom* g);

/* Host-only: 1 if dg_conv3x3_dgrad(g, ep, ...) takes the weight-stationary streaming kernel (one launch; all nine taps stay in
 * the registers of one workgroup per CU while dy streams through; bit-identical to the merged halo launch), else 0; negative =
 * dg_status.  The rule: bf16, stride 2, Cin = Cout = 128 with dense pixels (ldx = ldy = 128), no pixel shuffle; an epilogue that
 * is absent, plain, or mask_bits + mask_slope only; a dy row within the halo kernel's row-step limit (W/2 * 256 B < 8 MiB) and an
 * image of dx below 2 GiB.  ep may be NULL. */
int dg_conv3x3_dgrad_stream_eligible(const dg_conv_geom* g, const dg_epilogue* ep);

/* Process-wide A/B switch of that kernel: 0 = every stride-2 data gradient on the halo kernel, 1 = eligible calls stream
 * (default), n > 1 = as 1 with the launch capped at n workgroups (tests of the persistent walk at small shapes).  Negative
 * values count as 0.  Returns the previous value. */
int dg_set_s2_dgrad_stream(int on);

/* Derives the compute-precision weight packs from the fp32 MASTER, which is kept forward-packed and
 * padded as [CoutP][9][CinP] (tap = r*3+s; for a pixel-shuffle layer the host has already moved
 * output channel co=4c+2i+j to row (2i+j)*Cout/4 + c, torch PixelShuffle order, generator.py:73):
 *   kind 0 (forward pack): same layout cast to `dtype`;  kind 1 (dgrad pack): dst[ci][tap][co]. */
int dg_repack_conv_weights(int dtype, int kind, const float* master, void* dst, int CoutP, int CinP,
                           void* stream);
/* Data-gradient packs of a dense block's stacked ("virtual") convs: masters[k-1] = conv k's fp32 weight [F][9][k*F], k = 1..nconv
 * (generator.py:14-41).  dst = for j = 0..nconv-1 the kind-1 pack of the conv that takes the adjoints of convs j+1..nconv
 * ((nconv-j)*F channels) to the adjoint of slab slice j (F channels): dst_j[ci][tap][(k-j-1)*F + co] = W_k[co][tap][j*F + ci];
 * the packs concatenated, 9*F*F*nconv*(nconv+1)/2 elements of `dtype`. */
int dg_repack_dense_dgrad(int dtype, const float* const* masters, int nconv, int F, void* dst, void* stream);
/* Two helpers for layers with <= 2 real OUTPUT channels (generator conv3.2, generator.py:80), whose backward is HBM-bound:
 * dg_repack_conv_weights kind 2 = kind 1 with mirrored taps, the pack with which that layer's data gradient is a forward conv of
 * dy over its 2 real channels (im2col kernel); dg_wgrad_unswap: dw[co][t][ci] += tmp[ci][8-t][co], which folds a weight-gradient
 * launch with swapped operand roles (x := dy with 2 real channels, dy := x) back into the layer's gradient layout. */
int dg_wgrad_unswap(const float* tmp, float* dw, int CoutP, int CinP, void* stream);

/* ---- Linear family (replaces nn.Linear in critic.py:94-105) ---------------------------------- */

/* y[b][o] (fp32, pre-zeroed, ldy) += sum_k x[b][k] * w[o][k]; split-K with atomics. */
int dg_linear_fwd(int dtype, const void* x, int64_t ldx, const void* w, int64_t ldw, float* y,
                  int ldy, int B, int O, int64_t K, void* stream);
/* dx[b][k] = (sum_o dy[b][o] * w[o][k]) * LeakyReLU'(mask[b][k]);  dy fp32 [B][ldo]; dx in
 * out_dtype (DG_F32 or `dtype`); mask (optional) in `dtype`, same shape as dx. */
int dg_linear_dx(int dtype, int out_dtype, const float* dy, int ldo, const void* w, int64_t ldw,
                 void* dx, int64_t lddx, const void* mask, int64_t ldmask, float mask_slope, int B,
                 int O, int64_t K, void* stream);
/* dw[o][k] (fp32) += sum_b dy[b][o] * x[b][k]. */
int dg_linear_dw(int dtype, const float* dy, int ldo, const void* x, int64_t ldx, float* dw,
                 int64_t lddw, int B, int O, int64_t K, void* stream);
/* The same product for up to 128 rows and O <= 112 in ONE sweep over dw: the rows of every pass that contributes to
 * critic_loss.backward() (wasserstein.py:52: real, fake, penalty tangent) concatenated, so the 1.9 GB FC1 gradient
 * (critic.py:94-96) is written once per iteration instead of read-modify-written once per pass.
 * accumulate != 0: dw += ...; accumulate == 0: dw = ... (no zero-fill needed).  K % 4 == 0. */
int dg_linear_dw_wide(int dtype, const float* dy, int ldo, const void* x, int64_t ldx, float* dw,
                      int64_t lddw, int B, int O, int64_t K, int accumulate, void* stream);

/* ---- elementwise / reductions ----------------------------------------------------------------- */

/* out[r][c] = act(in_f32[r][c] + bias[c]) cast to out_dtype; optional mask multiply instead of act
 * (tangent pass).  Rows x C small matrices (critic head, critic.py:96-98). */
int dg_bias_act(int out_dtype, const float* in, int ldi, const float* bias, void* out, int ldo,
                int rows, int C, int has_act, float slope, const void* mask, int ldmask,
                float mask_slope, void* stream);
/* u[p][c] *= LeakyReLU'(y[p][c]) in place over a [rows x C] channel slice. */
int dg_mask_mul(int dtype, void* u, int64_t ldu, const void* y, int64_t ldy, int64_t rows, int C,
                float slope, void* stream);
/* out = a*x + b*y over [rows x C] slices (residual adds, generator.py:41,53,87). y may be NULL. */
int dg_axpby(int dtype, void* out, int64_t ldo, const void* x, int64_t ldx, float a, const void* y,
             int64_t ldy, float b, int64_t rows, int C, void* stream);
/* xhat[b] = alpha[b]*real[b] + (1-alpha[b])*fake[b]   (wasserstein.py:94). per_img = elements/image */
int dg_gp_interp(int dtype, const void* real, const void* fake, const float* alpha, void* xhat,
                 int B, int64_t per_img, void* stream);
/* The same interpolate for fields stored `ld` channels wide of which the first TWO are real: writes the COMPACT [pixel][2]
 * forms the critic's first layer reads fastest (dg_conv3x3_fwd / _wgrad with cin_real <= 2 take either layout) -- xhat_c, and
 * (optional, may be NULL) compact copies real_c / fake_c of the two inputs.  pix_per_img % 4 == 0. */
int dg_gp_interp_c2(int dtype, const void* real, const void* fake, int64_t ld, const float* alpha,
                    void* xhat_c, void* real_c, void* fake_c, int B, int64_t pix_per_img, void* stream);
/* out_c[b][pixel][0..1] = coef[b] * g[b][pixel][0..1]  (the penalty's v0 = dGP/dg, wasserstein.py:110-117 backward), g stored
 * `ld` channels wide, out_c compact. */
int dg_scale_rows_c2(int dtype, const void* g, int64_t ld, const float* coef, void* out_c, int B,
                     int64_t pix_per_img, void* stream);
/* ss[b] (fp32, pre-zeroed) += sum of squares of image b   (wasserstein.py:114), wave-shuffle reduce */
int dg_sumsq_rows(int dtype, const void* g, int B, int64_t per_img, float* ss, void* stream);
/* From ss[b]: n_b = sqrt(ss+1e-12); scalars[0] = gp_lambda*mean((n_b-1)^2)  (wasserstein.py:117);
 * coef[b] = weight * gp_lambda * (2/B_global) * (n_b-1)/n_b  (d/dg of weight*gp_ret). */
int dg_gp_finish(const float* ss, int B, int B_global, float gp_lambda, float weight, float* coef,
                 float* scalars, void* stream);
/* out[b] = coef[b] * g[b]  (per-image scale) */
int dg_scale_rows(int dtype, const void* g, const float* coef, void* out, int B, int64_t per_img,
                  void* stream);
/* L1 content loss (losses.py:51-53): acc[0] (fp32, pre-zeroed) += sum |a-b| over [rows x C] with C
 * real channels of ld-strided pixels; if grad: grad = grad_scale*sign(a-b) (+ addend if given). */
int dg_l1(int dtype, const void* a, int64_t lda, const void* b, int64_t ldb, int64_t rows, int C,
          float* acc, void* grad, int64_t ldg, float grad_scale, const void* addend, int64_t ldadd,
          void* stream);
/* acc[0] (fp32, pre-zeroed) += sum (a-b)^2 over [rows x C]  (content_MSELoss metric, losses.py:58-70; metrics pass
 * mlflow_epoch.py:53-63) */
int dg_sqdiff(int dtype, const void* a, int64_t lda, const void* b, int64_t ldb, int64_t rows, int C,
              float* acc, void* stream);
/* out[0] = scale * sum_{i<n} in[i*stride]  (means of critic outputs, wasserstein.py:46-47,74) */
int dg_sum_strided(const float* in, int n, int stride, float scale, float* out, void* stream);
/* fill fp32 buffer with a constant on a strided column (grad_outputs=ones, wasserstein.py:103) */
int dg_fill_col(float* buf, int rows, int ld, int col, float value, void* stream);

/* Adam (stage.py:63-64: lr 2.5e-4, betas (0.9,0.99), eps 1e-8, no weight decay) over a flat fp32
 * buffer; also refreshes the bf16 shadow copy when shadow != NULL.  grad_scale multiplies g first
 * (1/world_size after a sum all-reduce). */
int dg_adam(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr,
            float beta1, float beta2, float eps, int step, float grad_scale, void* stream);

/* Layout converters between the reference's NCHW fp32 tensors and native NHWC padded `dtype`. */
int dg_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int C, int H, int W, int Cpad,
                    void* stream);
int dg_nhwc_to_nchw(int dtype, const void* src, int64_t lds, float* dst, int N, int C, int H, int W,
                    void* stream);
/* fp32 -> dtype cast of n elements (weight shadows) */
int dg_cast(int dtype, const float* src, void* dst, int64_t n, void* stream);

/* ---- MS-SSIM of the per-step metrics pass.  Replaces `SSIM_Loss(x, y, device)`
 * (DoWnGAN/GAN/losses.py:12-38, called per batch from mlflow_tools/mlflow_epoch.py:53-63 at wasserstein.py:140), which
 * min-max normalises each channel over the batch and evaluates `pytorch_msssim.MS_SSIM(win_size=7, data_range=1,
 * channel=2)` (third-party, unpinned: the kernels follow its published algorithm; see oracle/msssim.py). */
#define DG_SSIM_MAX_CH 8
#define DG_SSIM_MAX_WIN 11
#define DG_SSIM_MAX_LEVELS 5
#define DG_MINMAX_PARTS 256
typedef struct dg_ssim_params {
  int win;                      /* Gaussian window length (reference: 7) */
  float g[DG_SSIM_MAX_WIN];     /* normalised 1-D Gaussian, sigma 1.5 (pytorch_msssim _fspecial_gauss_1d) */
  float C1, C2;                 /* (K1*data_range)^2, (K2*data_range)^2 with K = (0.01, 0.03) */
} dg_ssim_params;
typedef struct dg_msssim_combine {
  float inv_count[DG_SSIM_MAX_LEVELS];  /* 1 / ((H_l-win+1)*(W_l-win+1)) */
  float weight[DG_SSIM_MAX_LEVELS];     /* 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 */
} dg_msssim_combine;
/* per-channel min / max over `pixels` ld-strided pixels (first C channels): partial[DG_MINMAX_PARTS][C][2]
 * (losses.py:15-18, 23-26: x[:, c].min() / .max() over the whole batch).  NaN rule: a NaN pixel is skipped (fminf / fmaxf), so
 * the result is the min / max of the numbers; a channel with no number at all gives (+inf, -inf).  The NaN still reaches the
 * metric: dg_normalise_planar keeps it in its pixel, every window that covers it sums to NaN and dg_msssim_finish keeps a NaN
 * mean, so MS-SSIM of a batch with a NaN is NaN, as the reference's is.  A zero extreme may come back with either sign.
 * Channels >= C are never read. */
int dg_minmax_partial(int dtype, const void* x, int64_t pixels, int64_t ld, int C, float* partial, void* stream);
/* minmax[C][2] = {min, max} over the partials */
int dg_minmax_finish(const float* partial, int C, float* minmax, void* stream);
/* out[n][c][h][w] (planar fp32) = (x[n][h][w][c] - min_c) / (max_c - min_c)   (losses.py:20-21, 28-29) */
int dg_normalise_planar(int dtype, const void* x, int N, int H, int W, int64_t ld, int C, const float* minmax,
                        float* out, void* stream);
/* one scale of pytorch_msssim `_ssim`: sums[plane][0] += sum of the SSIM map, sums[plane][1] += sum of the CS map over
 * the 'valid' (H-win+1)x(W-win+1) window positions of every HxW plane of X, Y (planar fp32) */
int dg_ssim_level(const float* X, const float* Y, int planes, int H, int W, const dg_ssim_params* p, float* sums,
                  void* stream);
/* avg_pool2d(kernel 2, stride 2, padding = size % 2 per dim, padded zeros counted) between scales (`ms_ssim`): output (ho, wo)
 * averages rows 2 ho - H % 2 + {0, 1} and columns 2 wo - W % 2 + {0, 1}, so only the pad row / column on the TOP / LEFT is ever
 * inside a window; out is [planes][H / 2 + H % 2][W / 2 + W % 2].  H, W >= 2. */
int dg_avgpool2(const float* in, float* out, int planes, int H, int W, void* stream);
/* out[0] = sum over planes of prod_l relu(mean_l)^weight_l, mean_l = CS mean for l < levels-1, SSIM mean at the last
 * scale; sums is [levels][planes][2].  The caller divides by the (global) plane count (`size_average=True`).  relu is
 * torch.relu's: a negative mean gives 0, a NaN mean stays NaN (and makes out[0] NaN). */
int dg_msssim_finish(const float* sums, int levels, int planes, const dg_msssim_combine* cmb, float* out, void* stream);

/* Finite-difference physics metrics `divergence_loss` / `vorticity_loss` (DoWnGAN/GAN/losses.py:119-193; known answers in
 * DoWnGAN/GAN/tests/test_losses.py:75-116).  sums[10] (double) += {sum r, sum r^2, sum f, sum f^2, sum r*f} (the call ADDS to what
 * sums holds: zero it before the first call of a batch; column 0 of channel 0, row 0 of channel 1 and channels >= 2 are never read) of
 * the divergence (dudy + dvdx) of `hr` (r) and `fake` (f), then the same five of the vorticity (dvdx - dudy); channel 0 = u,
 * channel 1 = v, differences on the [1:, 1:] window.  The host forms MSE(r/std(r), f/std(f)) with the unbiased std. */
int dg_div_vort_sums(int dtype, const void* hr, int64_t ldhr, const void* fake, int64_t ldfake, int N, int H, int W,
                     double* sums, void* stream);

/* Data feed.  The reference keeps the whole train set on the device (stage.py:28-31) and lets a
 * shuffling `DataLoader` index it through `NetCDFSR.__getitem__` (dataloader.py:26-33, stage.py:69-72).  Here the set stays
 * resident in HBM as [n][H*W][c_real] in the compute dtype and one launch forms a minibatch in native layout:
 * dst[b][p][c] = src[idx[b]][p][c] for c < c_real, 0 for the padding channels up to c_pad.  idx: B int64 on the device. */
int dg_gather_samples(int dtype, const void* src, int64_t HW, int c_real, const int64_t* idx, int B, void* dst, int c_pad,
                      void* stream);

/* MXFP8 conv path (BASELINE.json configs[4]: "fp8 (CDNA4 fp8 MFMA) conv path"; reference math of the layers it serves:
 * DoWnGAN/networks/critic.py:25-88, the critic's seven 128..1024-channel convs).
 * dg_quant_mxfp8: rows x C values (C % 128 == 0, row stride `ld` elements, dtype DG_BF16 or DG_F32) -> OCP FP8 E4M3 bytes
 *   q[rows][ldq] + one E8M0 scale byte per block of 32 consecutive channels (OCP MX layout), scales[rows][C/32];
 *   scale = 2^(floor(log2 amax) - 8), elements = round-to-nearest-even(x / scale) saturated at +-448.
 *   The scale byte is max(0, exponent field of the block's largest magnitude - 8); fp32 / bf16 subnormal inputs keep their value.
 *   A block that holds a NaN or an Inf becomes 32 x 0x7F (E4M3 NaN) and gets scale byte 247 (exponent field 255 - 8) -- from
 *   this kernel, from dg_epilogue.out_q / out_qs and in the emulation alike (tests/test_fp8_quant_exact_*.py).
 *   Serves activations / adjoints (rows = pixels) and conv weight packs (rows = Nout * 9, C = Cred).
 * dg_conv3x3_fwd_f8 / dg_conv3x3_dgrad_f8: dg_conv3x3_fwd / _dgrad with both MFMA operands in that format and fp32
 *   accumulation; `g` describes the layer as for the bf16 calls (g->dtype = DG_BF16: the type of y / dx and of every
 *   epilogue operand), `q` carries the quantised source (xq, xs, pixel stride ldxq bytes) and weight pack (wq, ws: the
 *   forward pack [Cout][9][Cin] for _fwd, the data-gradient pack [Cin][9][Cout] for _dgrad).  Shapes: reduction channels a
 *   multiple of 128, more than 64 output channels, no pixel shuffle; anything else returns DG_ERR_BAD_SHAPE. */
typedef struct dg_f8_operands {
  const void* xq;   /* fp8 source, NHWC */
  const void* xs;   /* its scales [pixels][ldxs] (the first Cred/32 bytes of each row are used) */
  int64_t ldxq;     /* pixel stride of xq in bytes */
  int64_t ldxs;     /* scale bytes per pixel of xs; 0 = Cred/32 (dense); a multiple of 4; < 0 = xs is ONE row of Cred/32 exponents valid for every pixel (a uniform-scale source) */
  const void* wq;   /* fp8 weight pack [Nout][9][Cred] */
  const void* ws;   /* its scales [Nout][9][Cred/32] */
} dg_f8_operands;
/* out[b] = min(254, E8M0 exponent byte of the magnitude in amax[b] (floor(log2) - 8 + 127, >= 0) + margin), b < nblocks <= 64, and amax[b] = 0:
 * turns the census a first-layer launch kept (dg_epilogue.out_amax) into the exponents of the next pass's uniform-scale copy -- the same
 * values dg_block_exp_max derives from the MXFP8 scale bytes of that tensor. */
int dg_exp_from_amax(void* amax, int nblocks, int margin, void* out, void* stream);

/* out[b] = min(254, max over rows r of scales[r * ld + b] + margin), b < nblocks: the largest MXFP8 block exponent a tensor's
 * 32-channel block b reached anywhere (scales = the E8M0 bytes dg_quant_mxfp8 / dg_epilogue.out_qs wrote) -- the per-block exponent
 * of the uniform-scale copy (dg_epilogue.out_u) of the NEXT pass over the same tensor.  nblocks <= 64, a multiple of 4; `scratch`
 * = 64 * DG_EXP_BATCH_MAX dwords of device memory the caller owns, ZERO on entry and left zero (one per stream that calls this
 * concurrently). */
int dg_block_exp_max(const void* scales, int64_t rows, int64_t ld, int nblocks, int margin, void* out, void* scratch, void* stream);

/* The same for up to DG_EXP_BATCH_MAX tensors in one launch (the fp8 train step refreshes a dozen exponent tables per critic pass);
 * scratch = 64 * DG_EXP_BATCH_MAX dwords, zero on entry and left zero. */
#define DG_EXP_BATCH_MAX 16
typedef struct dg_exp_batch {
  const void* scales[DG_EXP_BATCH_MAX];
  int64_t rows[DG_EXP_BATCH_MAX];
  int64_t ld[DG_EXP_BATCH_MAX];
  int nblocks[DG_EXP_BATCH_MAX];
  void* out[DG_EXP_BATCH_MAX];
  int n;
} dg_exp_batch;
int dg_block_exp_max_batch(const dg_exp_batch* b, int margin, void* scratch, void* stream);

/* Stand-alone form of dg_epilogue.out_u: q[r][c] = E4M3(src[r][c] / 2^(exps[c / 32] - 127)) (saturated at +-448; a block holding a
 * NaN / Inf becomes 32 x NaN), for tensors that do not come out of a conv epilogue (the critic's last adjoint, written by the FC's
 * input gradient).  src bf16 / fp32 [rows][ld], C % 128 == 0, q [rows][ldq] bytes.  Every exponent byte 0 .. 254 (2^-127 .. 2^127,
 * everything dg_block_exp_max / dg_exp_from_amax can return) is served against every finite value, here and in out_u: a quotient
 * past +-448 saturates however large it is, one below 2^-10 becomes zero. */
int dg_quant_uniform(int src_dtype, const void* src, int64_t rows, int64_t ld, int C, const void* exps, void* q, int64_t ldq, void* stream);

int dg_quant_mxfp8(int src_dtype, const void* src, int64_t rows, int64_t ld, int C, void* q, int64_t ldq, void* scales,
                   int64_t ldqs, void* stream);   /* ldqs: scale bytes per row, 0 = C/32 */
int dg_conv3x3_fwd_f8(const dg_conv_geom* g, const dg_epilogue* ep, const dg_f8_operands* q, void* y, void* stream);
int dg_conv3x3_dgrad_f8(const dg_conv_geom* g, const dg_epilogue* ep, const dg_f8_operands* q, void* dx, void* stream);

/* Dataset preprocessing of the data feed.
 * dg_moments: acc[3] (double) += { sum, sum of squares, count } over the non-NaN elements of x[n] (the call ADDS to what acc holds,
 *   so a record is accumulated chunk by chunk from a zeroed acc; an Inf is an element like any other: counted, sums Inf) -- the
 *   moments behind `xr_standardize_array` (DoWnGAN/helpers/gen_experiment_datasets.py:195-201: da.mean(skipna=True),
 *   da.std(skipna=True), population std), accumulated chunk by chunk over a field's whole record.  x 16-byte aligned.
 * dg_stage_fields: dst[p][k] = (plane[k][p] - mean[k]) * inv_std[k] for p < npix, k < c -- the standardisation itself fused
 *   with the [time, var, lat, lon] staging of DoWnGAN/GAN/stage.py:28-31, written as the HBM-resident [n][H*W][c] store that
 *   dg_gather_samples reads.  A field that must not be standardised (the binary `land_sea_mask`,
 *   gen_experiment_datasets.py:208-209) is passed with mean 0 and inv_std 1.  NaNs stay NaNs, as in the reference. */
#define DG_MAX_FIELDS 8
typedef struct dg_field_planes {
  const float* plane[DG_MAX_FIELDS]; /* c device pointers, each [npix] fp32 */
  float mean[DG_MAX_FIELDS];
  float inv_std[DG_MAX_FIELDS];
  int c;
} dg_field_planes;
int dg_moments(const float* x, int64_t n, double* acc, void* stream);
int dg_stage_fields(int dtype, const dg_field_planes* f, int64_t npix, void* dst, void* stream);

/* Frequency-separation variant (DoWnGAN/GAN/wasserstein_fs.py:36-46,73-86, hyperparams.py:31-35):
 * low = AvgPool2d(5, stride 1)(ReplicationPad2d(2)(x)) and/or high = x - low of an NHWC tensor (C padded channels,
 * multiple of 8); either output may be NULL. */
int dg_lowpass5(int dtype, const void* x, int64_t ldx, int N, int H, int W, int C, void* low, int64_t ldl, void* high,
                int64_t ldh, void* stream);
/* out = low^T(g): the adjoint of the operator above (what autograd applies in the reference's `g_loss.backward()`,
 * wasserstein_fs.py:88, to reach `fake` through `fake_low` and `fake_high`). */
int dg_lowpass5_adjoint(int dtype, const void* g, int64_t ldg, int N, int H, int W, int C, void* out, int64_t ldo,
                        void* stream);

/* ---- debugging aids (off by default; csrc/debug.hip) ----------------------------------------------------------------
 * dg_set_deterministic_workspace: the split-K weight gradients (dg_conv3x3_wgrad, _wgrad_dense) and the small reductions
 *   (dg_colsum, dg_sumsq_rows, dg_l1, dg_sqdiff, dg_linear_fwd) accumulate partial results with fp32 atomics, whose order -- and
 *   so the last bits of every gradient -- differs from run to run.  With a caller-owned device workspace registered here
 *   (>= 1 MiB, 16-byte aligned; NULL switches the mode off again) each of those launches writes its partials side by side into
 *   the workspace and adds them to the target in a fixed order: results are bit-identical between runs.  Process-wide; the
 *   workspace must stay alive while registered and serves one stream at a time.  A launch that needs more room than the
 *   workspace has runs with fewer splits (slower, same guarantee).
 * dg_count_nonfinite: counts[i] = number of NaN / Inf elements of buffer i -- the stand-in for the reference's global
 *   torch.autograd.set_detect_anomaly(True) (DoWnGAN/GAN/wasserstein.py:13), run once per iteration by
 *   TrainEngine(check_finite=True) instead of after every op. */
#define DG_FINITE_MAX 8
typedef struct dg_finite_bufs {
  const void* ptr[DG_FINITE_MAX];
  int64_t n[DG_FINITE_MAX];      /* elements */
  int dtype[DG_FINITE_MAX];      /* DG_F32 or DG_BF16 */
  int nbuf;
} dg_finite_bufs;
int dg_set_deterministic_workspace(void* ws, int64_t bytes);
int dg_deterministic(void);      /* 1 while a workspace is registered */
int dg_count_nonfinite(const dg_finite_bufs* bufs, uint32_t* counts, void* stream);

/* ---- EOF analysis (csrc/eof.hip) -------------------------------------------------------------------------------------
 * Empirical orthogonal functions = one PCA per channel of a time series of fields: the reference fits sklearn `PCA` on the host
 * (DoWnGAN/helpers/prep_gan.py:226-255) and projects / reconstructs with torch in `eof_loss` (DoWnGAN/GAN/losses.py:72-116)
 * and `low_pass_eof_batch` (losses.py:196-228).  Here the fit is mean -> centred Gram (f32 MFMA) -> host eigh of the T x T
 * Gram -> components, and projection / reconstruction stream the fields once.
 * Fields are read through one strided descriptor: element (t, c, p), p = h*W + w, sits at base + t*ld_t + c*ld_c + p*ld_p
 * (ELEMENTS of `dtype`, DG_F32 or DG_BF16; bf16 is widened on load).  NCHW tensors: ld_p = 1, ld_c = H*W; the resident feed's
 * [n, H, W, c] store: ld_p = c, ld_c = 1.  C <= DG_EOF_MAX_C.  Components E are fp32 with unit pixel stride: E[c][k][p] at
 * E + k*ld_k + c*ld_c + p ([C, K, P]: ld_k = P, ld_c = K*P; the reference's [K, C, P]: ld_k = C*P, ld_c = P).
 * All reductions are deterministic: fixed-order sums, no float atomics; two calls on the same data are bit-identical.
 *
 * dg_eof_mean: mu[c][p] = mean over t (fp64 accumulation).
 * dg_eof_gram: G[c][i][j] = sum_p (x[i,c,p] - mu[c,p]) (x[j,c,p] - mu[c,p]) as fp64 [C][T][T].  Centring is fused into the
 *   operand load; upper-triangle 64 x 64 tiles only, mirrored.  The P range is split into `nslice` slices: ws holds
 *   nslice * ntiles * C * 4096 fp32 partial slabs, ntiles = nb (nb + 1) / 2, nb = ceil(T / 64); slices are summed in order in
 *   fp64.  1 <= nslice <= ceil(P / 64).
 * dg_eof_components: E[c][k][p] = sum_t A[c][t][k] (x[t,c,p] - mu[c,p]) for k < K, A fp32 [C][T][lda] (lda = K rounded up to a
 *   multiple of 16, zero beyond K).  amax[c][k] (pre-zeroed) receives the position of the entry of largest magnitude of row
 *   (c, k), ties to the lowest p, as the key (|E| bits << 32) | (0xffffffff - p) (integer max: order-independent).
 * dg_eof_flip: negates every row (c, k) of E whose entry at the amax position is negative (sklearn's sign rule:
 *   svd_flip(u_based_decision=False) makes the entry of largest magnitude of every component positive).
 * dg_eof_project: Z[b][c][k] = sum_p (y[b,c,p] - m[c,p]) E[c][k][p] (fp32 [B][C][K], B = y->T; m NULL = uncentred).  A
 *   split-P product on the Gram kernel's machinery: ws holds nslice * ceil(B/64) * ceil(K/64) * C * 4096 fp32.
 * dg_eof_reconstruct: out[b][c][p] = sum_k Z[b][c][k] E[c][k][p] (+ mu[c][p] when mu is not NULL), fp32 NCHW [B][C][P]; Z is
 *   fp32 [B][C][K]. */
#define DG_EOF_MAX_C 8
#define DG_EOF_MAX_K 64
typedef struct dg_eof_fields {
  const void* base;
  int dtype;
  int T, C, P;
  int64_t ld_t, ld_c, ld_p;
} dg_eof_fields;
int dg_eof_mean(const dg_eof_fields* x, float* mu, void* stream);
int dg_eof_gram(const dg_eof_fields* x, const float* mu, int nslice, float* ws, double* G, void* stream);
int dg_eof_components(const dg_eof_fields* x, const float* mu, const float* A, int K, float* E, int64_t ld_k, int64_t ld_c,
                      unsigned long long* amax, void* stream);
int dg_eof_flip(float* E, int C, int K, int P, int64_t ld_k, int64_t ld_c, const unsigned long long* amax, void* stream);
int dg_eof_project(const dg_eof_fields* y, const float* m, const float* E, int K, int64_t ld_k, int64_t ld_c, int nslice,
                   float* ws, float* Z, void* stream);
int dg_eof_reconstruct(const float* Z, int B, int C, int K, const float* E, int64_t ld_k, int64_t ld_c, int P, const float* mu,
                       float* out, void* stream);

/* ---- Radially averaged power spectra (csrc/spectra.hip) ----------------------------------------------------------------
 * The standard per-scale diagnostic of a downscaling generator: the radially averaged power spectral density (RAPSD) of real
 * and generated fields.  Fields are square, N x N with N a power of two, 16 <= N <= DG_RAPSD_MAX_N, read through the EOF
 * descriptor with P = N*N, p = h*N + w (NCHW fp32, the resident feed's [n, H, W, c] store, or the generator's padded NHWC
 * output: ld_p = padded channel count, C = real channels; bf16 is widened on load).  For one field x:
 *   P[u][v] = |FFT2(x)[u][v]|^2 / N^2, with signed integer frequencies u, v in [-N/2, N/2);
 *   ring k holds (u, v) with (2k-1)^2 <= 4 (u^2 + v^2) < (2k+1)^2, evaluated exactly in integers; K = N/2 + 1 rings, pixels
 *   of rings k > N/2 (the corners) are dropped; no windowing, no mean removal (ring 0 holds the mean's power);
 *   S[k] = mean of P over ring k.
 * Row pass: two real rows as one complex N-point FFT (Stockham radix-4 in LDS, fp32 twiddles rounded once from double), half
 * spectra written transposed; column pass: N-point FFT per line u, power with the Hermitian weight, ring sums per workgroup;
 * the partials are summed in a fixed order in fp64.  No float atomics: two calls on the same data are bit-identical.
 *
 * dg_rapsd_ws_bytes: workspace bytes of dg_rapsd for T fields of C channels (0 for an invalid shape); ~8 (N/2 + 1) N bytes per
 *   field (the half spectra) plus small fp64 partials.
 * dg_rapsd: per_field[t][c][k] (fp64 [T][C][N/2+1], may be NULL) and sum[c][k] = sum over t of per_field[t][c][k] in t order
 *   (fp64 [C][N/2+1], may be NULL).  x->P must equal N*N, x->C <= DG_EOF_MAX_C.
 * dg_rapsd_ring_counts: host-side, counts[k] = number of frequencies (u, v) in ring k, k = 0..N/2 (the divisors the kernels use). */
#define DG_RAPSD_MAX_N 2048
size_t dg_rapsd_ws_bytes(int T, int C, int N);
int dg_rapsd(const dg_eof_fields* x, int N, void* ws, double* per_field, double* sum, void* stream);
int dg_rapsd_ring_counts(int N, int64_t* counts);

/* ---- Cross spectra (csrc/spectra.hip) ----------------------------------------------------------------------------------
 * Down to which scale is a generated field the same field as the truth?  For a pair of square fields a, b (N x N as above, read
 * through two independent EOF descriptors: each side has its own layout and dtype), A = FFT2(a), B = FFT2(b):
 *   Paa[u][v] = |A|^2 / N^2,  Pbb[u][v] = |B|^2 / N^2,  Cab[u][v] = Re(A conj(B)) / N^2 = (A.re B.re + A.im B.im) / N^2
 * averaged over the rings of dg_rapsd (the same ring test, counts = dg_rapsd_ring_counts, corners dropped).  Output per
 * (field, channel): three ring means [3][K], K = N/2 + 1, plane 0 = Paa, 1 = Pbb, 2 = Cab.  The imaginary part of the cross
 * spectrum is not stored: rings are symmetric under (u, v) -> (-u, -v), so for real fields it sums to zero.  From the planes
 * follow per wavenumber the coherence Cab / sqrt(Paa Pbb) and the spectrum of the error a - b, Paa + Pbb - 2 Cab.
 * Row pass: dg_rapsd's, once per side, into two half-spectrum buffers; column pass: per slice of lines u, side a's FFT kept in
 * LDS next to side b's, the power as fmaf(X.re, X.re, X.im * X.im) and the co-spectrum as fmaf(A.re, B.re, A.im * B.im), each
 * times 1 / N^2 and the Hermitian weight, ring sums in fp64 in dg_rapsd's order.  Hence, bit for bit: planes 0 and 1 equal
 * dg_rapsd of a and of b, plane 2 is symmetric in (a, b), and plane 2 of (a, a) equals plane 0.  No float atomics: every sum
 * runs in a fixed order and two calls on the same data are bit-identical.
 *
 * dg_cross_rapsd_ws_bytes: workspace bytes of dg_cross_rapsd for T pairs of C channels (0 for an invalid shape); ~16 (N/2 + 1) N
 *   bytes per field (both sides' half spectra) plus small fp64 partials.
 * dg_cross_rapsd: per_field[t][c][plane][k] (fp64 [T][C][3][K], may be NULL) and sum[c][plane][k] = sum over t in t order (fp64
 *   [C][3][K], may be NULL).  a and b must agree in T, C and P = N*N (DG_ERR_BAD_SHAPE otherwise; dtypes other than fp32 / bf16:
 *   DG_ERR_BAD_DTYPE; both before any launch). */
size_t dg_cross_rapsd_ws_bytes(int T, int C, int N);
int dg_cross_rapsd(const dg_eof_fields* a, const dg_eof_fields* b, int N, void* ws, double* per_field, double* sum, void* stream);

/* ---- Helmholtz spectra (csrc/spectra.hip) -------------------------------------------------------------------------------
 * What kind of motion carries the variance at a given scale?  The kinetic energy spectrum of a vector field (u, v) = channels
 * (cu, cv) of the descriptor, split into its rotational and divergent parts.  N x N fields as above; scale[0], scale[1]: a factor
 * per component (finite, non-zero, the sign allowed), U = scale[0] FFT2(u), V = scale[1] FFT2(v); kx = the signed integer
 * frequency along W (the last axis), ky along H, k2 = kx^2 + ky^2:
 *   ke  = (|U|^2 + |V|^2)  / (2 N^2)
 *   div = |kx U + ky V|^2  / (2 k2 N^2)    (0 where k2 = 0)
 *   rot = |kx V - ky U|^2  / (2 k2 N^2)    (0 where k2 = 0)
 * averaged over the rings of dg_rapsd; rot + div = ke on every ring k >= 1.  The first component points along increasing column
 * index, the second along increasing row index; a field whose first channel points along H is the same call with cu, cv
 * exchanged, rows that run the other way are the same call with scale[1] negated.  The split is NOT invariant under
 * per-channel scaling: on standardised channels pass their standard deviations.
 * For a pair (a, b), with R = kx V - ky U and D = kx U + ky V of each side, also
 *   co_rot = Re(Ra conj Rb) / (2 k2 N^2),  co_div = Re(Da conj Db) / (2 k2 N^2),   |co_x| <= sqrt(x_a x_b) per ring.
 * Nyquist rule: a point of the half spectrum with u = N/2 or v = N/2 stands for two frequencies whose cross terms
 * 2 kx ky Re(U conj V) cancel in the ring sum, so it contributes div ~ kx^2 |U|^2 + ky^2 |V|^2, rot ~ kx^2 |V|^2 + ky^2 |U|^2
 * (the co-planes: the corresponding real parts); for real fields this equals the full-spectrum definition above.
 * Row pass: dg_rapsd's, once per component and side; column pass: both components' lines of a slice in LDS, the planes formed
 * per point in fp32, ring sums in fp64 in dg_rapsd's order.  No float atomics: two calls on the same data are bit-identical;
 * planes 0-5 of dg_helmholtz_cross equal dg_helmholtz of a and of b bit for bit, and (a, a) gives co_rot = rot, co_div = div.
 *
 * dg_helmholtz_ws_bytes / dg_helmholtz_cross_ws_bytes: workspace bytes for T fields (pairs) (0 for an invalid shape); ~16 (32)
 *   (N/2 + 1) N bytes per field (pair): the half spectra of both components (of both sides) plus small fp64 partials.
 * dg_helmholtz: per_field[t][plane][k] (fp64 [T][3][K], planes ke, rot, div; may be NULL) and sum[plane][k] over t in t order
 *   (fp64 [3][K], may be NULL).  cu != cv, both < x->C; x->P = N*N.
 * dg_helmholtz_cross: per_field fp64 [T][8][K], sum fp64 [8][K], planes ke_a, rot_a, div_a, ke_b, rot_b, div_b, co_rot, co_div.
 *   a and b agree in T, C and P; layouts and dtypes (fp32 / bf16) are independent.
 * Bad shapes, channel indices or scales: DG_ERR_BAD_SHAPE; other dtypes: DG_ERR_BAD_DTYPE; both before any launch. */
size_t dg_helmholtz_ws_bytes(int T, int N);
int dg_helmholtz(const dg_eof_fields* x, int cu, int cv, const float scale[2], int N, void* ws, double* per_field, double* sum,
                 void* stream);
size_t dg_helmholtz_cross_ws_bytes(int T, int N);
int dg_helmholtz_cross(const dg_eof_fields* a, const dg_eof_fields* b, int cu, int cv, const float scale[2], int N, void* ws,
                       double* per_field, double* sum, void* stream);

/* ---- Value histograms (csrc/histogram.hip) ------------------------------------------------------------------------------
 * The distribution check of a downscaling generator: per-channel histograms of real and generated fields, read in place
 * through the EOF descriptor (any T, P; NCHW fp32 / bf16, the resident feed's [n, H, W, c] store, the generator's padded NHWC
 * output: ld_p = padded channel count, C = real channels).  Every operation below is one correctly rounded fp32 operation,
 * never contracted:
 *   y_c = (x_c * scale[c]) + offset[c]                     input channel c (scale 1, offset 0: y = x, -0 read as +0)
 *   s   = sqrt(y_u * y_u + y_v * y_v)                       speed_u >= 0: appended as output channel C (nout = C + 1)
 *   t   = (y - lo[j]) * inv_w[j]                            output channel j; inv_w = fp32(nbins / (hi - lo)) rounded once
 *   bin = NaN -> nbins + 2;  t < 0 (-inf too) -> 0;  t >= nbins (+inf too) -> nbins + 1;  else 1 + (int)t
 * Subnormals are kept.  counts: int64 [nout][nbins + 3] (underflow, nbins interior bins, overflow, NaN), exact for any T * P;
 * moments: fp64 [nout][2] (sum, sum of squares of the finite y); extrema: fp32 [nout][2] (min, max of the finite y).  dg_hist
 * ACCUMULATES: counts and moments +=, extrema min / max (the caller initialises them).  Each workgroup keeps its histogram in
 * LDS (ds_add_u32) and adds the non-zero bins to counts with 64-bit integer atomics; moments and extrema go through per-
 * workgroup partials summed in workgroup order.  No float atomics: two calls on the same data are bit-identical.
 *
 * dg_hist_ws_bytes: workspace bytes of dg_hist for these fields (0 for an invalid descriptor or spec).
 * dg_hist_host_bins: host-side, the same transform and bin rule for x fp32 [C][n] (planar): bins int32 [nout][n]. */
#define DG_HIST_MAX_BINS 4096
#define DG_HIST_MAX_OUT (DG_EOF_MAX_C + 1)
typedef struct dg_hist_spec {
  int nbins;                       /* 1 .. DG_HIST_MAX_BINS, every output channel */
  int speed_u, speed_v;            /* input channels of the speed channel, or -1, -1: none */
  float lo[DG_HIST_MAX_OUT];       /* per output channel, finite */
  float inv_w[DG_HIST_MAX_OUT];    /* per output channel, finite and > 0 */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];   /* per input channel */
} dg_hist_spec;
size_t dg_hist_ws_bytes(const dg_eof_fields* x, const dg_hist_spec* s);
int dg_hist(const dg_eof_fields* x, const dg_hist_spec* s, void* ws, int64_t* counts, double* moments, float* extrema,
            void* stream);
int dg_hist_host_bins(const dg_hist_spec* s, const float* x, int C, int64_t n, int32_t* bins);

/* ---- Per-gridpoint statistics (csrc/gridstats.hip) -----------------------------------------------------------------------
 * Where on the grid is the generator wrong: running per-pixel statistics over the fields t of one series a, or of two series
 * a (real) and b (generated) of equal T, C, P, each read in place through the EOF descriptor (NCHW fp32 / bf16, the resident
 * feed's [n, H, W, c] store, the generator's padded NHWC output; a and b may differ in layout and dtype).  The output values
 * are those of the value histograms (the same code, csrc/hist_common.h), every fp32 operation rounded once, never contracted:
 *   y_c = (x_c * scale[c]) + offset[c]                     output channel j = c
 *   s   = sqrt(y_u * y_u + y_v * y_v)                       speed_u >= 0: appended as output channel C (nout = C + 1)
 *   valid <=> y finite;   u = (double)y - (double)pivot[j]
 * Per series, over the valid t of output channel j and pixel p: n (int32), S1..S4 = sum u, u^2, u^3, u^4 (fp64), min and max
 * of y (fp32), and over ALL t the exceedance counts E_k = #{y > thr[j][k]}, k < nthr (an fp32 compare: NaN is false, +inf is
 * true).  Paired, over the t where both values are valid: n_ab, D1 = sum d, DA = sum |d|, D2 = sum d^2 with
 * d = (double)y_b - (double)y_a, and X = sum u_a u_b.
 * Everything ACCUMULATES into caller-owned device arrays, the pixel index fastest (the caller initialises them: zeros, and
 * +inf / -inf for the minima / maxima).  Rows per output channel:
 *   sums    fp64  [nout][NS][P]   one series (NS = 4):  S1 S2 S3 S4
 *                                 paired    (NS = 12): a.S1 a.S2 a.S3 a.S4  b.S1 b.S2 b.S3 b.S4  D1 DA D2 X
 *   extrema fp32  [nout][NE][P]   one series (NE = 2):  min max;   paired (NE = 4): a.min a.max b.min b.max
 *   counts  int32 [nout][NC][P]   one series (NC = 1 + nthr):      n  E_0 .. E_{nthr-1}
 *                                 paired    (NC = 3 + 2 nthr):     n_a n_b n_ab  a.E_0 .. a.E_{nthr-1}  b.E_0 .. b.E_{nthr-1}
 * A thread owns its pixels and walks the fields in t order with its state in registers, so there are no atomics at all: the
 * integer counts and the extrema are exact, and two calls on the same data are bit-identical.  When P alone does not fill the
 * chip the t range is cut into S = dg_gridstats_slices(T, P) contiguous slices, slice s = fields [s T / S, (s + 1) T / S);
 * each slice's partial state goes to the workspace and a second kernel adds the slices in slice order into the accumulators.
 * The bits of the fp64 sums therefore depend on S, a function of (T, P) only:
 *   nb = ceil(P / 256);   S = 1 when nb >= 1024, else max(1, min(ceil(1024 / nb), floor(T / 16))).
 *
 * dg_gridstats_ws_bytes: workspace bytes of one call (0 for an invalid descriptor or spec; `paired` != 0: two series).
 * dg_gridstats_slices: host-side, the S above (0 for T < 1 or P < 1).
 * dg_gridstats: b NULL = one series.  ws may be NULL when S = 1. */
#define DG_GRID_MAX_THR 4
typedef struct dg_grid_spec {
  int speed_u, speed_v;            /* input channels of the speed channel, or -1, -1: none */
  int nthr;                        /* 0 .. DG_GRID_MAX_THR thresholds per output channel */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];   /* per input channel, finite */
  float pivot[DG_HIST_MAX_OUT];    /* per output channel, finite */
  float thr[DG_HIST_MAX_OUT][DG_GRID_MAX_THR];       /* per output channel, the first nthr finite */
} dg_grid_spec;
size_t dg_gridstats_ws_bytes(const dg_eof_fields* a, int paired, const dg_grid_spec* s);
int dg_gridstats_slices(int T, int P);
int dg_gridstats(const dg_eof_fields* a, const dg_eof_fields* b, const dg_grid_spec* s, void* ws, double* sums, float* extrema,
                 int32_t* counts, void* stream);

/* ---- Fractions skill score (csrc/fss.hip) -----------------------------------------------------------------------------------
 * At which neighbourhood size does the generated field put threshold exceedances where the real field has them (Roberts & Lean
 * 2008): the score that does not punish a displaced feature twice.  Fields are H x W, read through the EOF descriptor with
 * P = H*W, p = h*W + w; series a (real) and b (generated) have equal T, C, P and may differ in layout and dtype (NCHW fp32 /
 * bf16, the resident feed's [n, H, W, c] store, the generator's padded NHWC output).  The output values y are those of the
 * value histograms and the per-gridpoint statistics (the same code, csrc/hist_common.h): C components plus the optional speed
 * channel appended last (nout = C + 1).  For output channel j, threshold k (thr[j][k], fp32) and window side n = win[s] (odd):
 *   masks          I_a[t,p] = (y_a > thr[j][k]), an fp32 compare: NaN is false, +inf is true, equality is false; I_b likewise
 *   window counts  c_a[t,h,w] = number of set I_a in rows h-r .. h+r, columns w-r .. w+r, r = (n-1)/2; positions outside the
 *                  grid count zero (zero padding); c_b likewise
 *   sums           D = sum (c_a - c_b)^2,  A = sum c_a^2,  B = sum c_b^2   over all t and pixels, exact integers
 *   base rates     N_a = sum I_a,  N_b = sum I_b
 *   score          FSS = 1 - D / (A + B) (the 1/n^2 of the fractions cancels; NaN when A + B = 0), formed on the host from the
 *                  integers
 * One kernel reads every pixel of a series once, forms the masks of all (j, k) and writes their row prefix counts (wave ballots
 * and popcounts) into one uint32 plane per (t, series, j, k) of the workspace; a second accumulates the planes down the columns
 * into summed-area tables (entries <= P <= 2^22); a third takes the four clipped corners of both tables per pixel and scale,
 * squares in 64-bit, reduces per workgroup and adds with 64-bit integer atomics into per-field slots of the workspace; the last
 * adds the slots to the accumulators.  No float after the compare and only integer atomics: the results are exact and two calls
 * on the same data are bit-identical.
 *
 * dg_fss_bound: host-side, H*W * (min(win, H) * min(win, W))^2, the most one field adds to D, A or B; 0 when H, W or win is
 *   invalid or the value exceeds 2^62.
 * dg_fss_ws_bytes: workspace bytes of one call (0 for an invalid descriptor, grid or spec): 8 nout nthr P bytes per field plus
 *   the per-field slots.
 * dg_fss: sums int64 [nout][nthr][nscale][3] (D A B) and rates int64 [nout][nthr][2] (N_a N_b) ACCUMULATE (the caller zeroes
 *   them and owns their headroom); per_field int64 [T][nout][nthr][nscale][3] is overwritten and may be NULL.  Rejected before
 *   any launch: descriptors that differ in T / C / P, P != H*W, H or W above DG_FSS_MAX_SIDE, an even, unsorted or out-of-range
 *   win, a non-finite thr / scale / offset, a scale whose dg_fss_bound is 0, and T * max_s dg_fss_bound > 2^62 (one call cannot
 *   overflow).
 * dg_fss_host: host-side, the same definition for one field pair, planar fp32 [C][H][W]; sums and rates +=. */
#define DG_FSS_MAX_THR 4
#define DG_FSS_MAX_SCALES 8
#define DG_FSS_MAX_SIDE 2048            /* H, W */
typedef struct dg_fss_spec {
  int speed_u, speed_v;                 /* input channels of the speed channel, or -1, -1: none */
  int nthr, nscale;                     /* 1 .. MAX each */
  int win[DG_FSS_MAX_SCALES];           /* odd, 1 <= win <= 2*DG_FSS_MAX_SIDE - 1, strictly increasing */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];   /* per input channel, finite */
  float thr[DG_HIST_MAX_OUT][DG_FSS_MAX_THR];        /* per output channel, the first nthr finite */
} dg_fss_spec;
size_t dg_fss_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_fss_spec* s);
int dg_fss(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_fss_spec* s, void* ws, int64_t* sums,
           int64_t* rates, int64_t* per_field, void* stream);
int dg_fss_host(const dg_fss_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* sums, int64_t* rates);
int64_t dg_fss_bound(int H, int W, int win);

/* ---- Intensity-scale verification (csrc/iscale.hip) --------------------------------------------------------------------------
 * At which spatial scale, for which intensity, does the error of the generated field live (Casati, Ross & Stephenson 2004; the
 * energies of Casati 2010): the error of the thresholded fields split into orthogonal 2-D Haar components, one per dyadic scale,
 * so that the mean squared error adds up over the scales.  Fields, series, output values y and masks are those of the fractions
 * skill score above (the same code, csrc/hist_common.h): I_a[t,p] = (y_a > thr[j][k]), an fp32 compare (NaN false, +inf true,
 * equality false), I_b likewise.  Let n be the smallest integer with 2^n >= max(H, W); the masks are zero outside the grid, on
 * the 2^n x 2^n square anchored at pixel (0, 0).  For level l = 0 .. n the square is tiled into aligned blocks of side 2^l, and
 * with S_l(X, block) the sum of X over a block, per output channel j, threshold k and level l:
 *   sums           D_l = sum (S_l(I_b) - S_l(I_a))^2,  A_l = sum S_l(I_a)^2,  B_l = sum S_l(I_b)^2   over all t and blocks, exact
 *                  integers; D_0 = the disagreeing pixels, A_0 = N_a, B_0 = N_b (dg_fss's D, A, B at window 1)
 *   components     formed on the host from the integers, E = D, A or B: the Haar (mother) component of the features of side
 *                  2^(l-1) is E_(l-1) / 4^(l-1) - E_l / 4^l, l = 1 .. n, the father component E_n / 4^n; they sum to E_0
 * One kernel reads every pixel of both series once: a workgroup of four waves owns a 64 x 64 tile, takes the masks of all (j, k) of a row as wave
 * ballots (one 64-bit word per row and side, kept in LDS), counts the levels 0 .. 6 with popcounts, packed adds and xor shuffles
 * and adds them with 64-bit integer atomics into per-field slots of the workspace; the tile totals (two counts <= 4096) go to
 * the workspace, and for n > 6 a second kernel builds the levels 7 .. n over the <= 32 x 32 tiles in LDS, one workgroup per
 * (t, j, k); the last adds the slots to the accumulators.  No per-pixel workspace, no float after the compare and only integer
 * atomics: the results are exact and two calls on the same data are bit-identical.
 *
 * dg_iscale_levels: host-side, n + 1 (the number of levels 0 .. n); 0 when H or W is outside 1 .. DG_ISCALE_MAX_SIDE.
 * dg_iscale_bound: host-side, 16^n, the most one field adds to any entry (2^44 at 2048 x 2048); 0 when H or W is invalid.
 * dg_iscale_ws_bytes: workspace bytes of one call (0 for an invalid descriptor, grid or spec): the per-field slots and one
 *   4-byte total per (t, j, k, tile).
 * dg_iscale: sums int64 [nout][nthr][n+1][3] (D A B) ACCUMULATE (the caller zeroes them and owns their headroom); per_field
 *   int64 [T][nout][nthr][n+1][3] is overwritten and may be NULL.  Rejected before any launch: descriptors that differ in
 *   T / C / P, P != H*W, H or W above DG_ISCALE_MAX_SIDE, a non-finite thr / scale / offset, and T * dg_iscale_bound > 2^62 (one
 *   call cannot overflow).
 * dg_iscale_host: host-side, the same definition by loops over the blocks for one field pair, planar fp32 [C][H][W]; sums
 *   [nout][nthr][n+1][3] +=. */
#define DG_ISCALE_MAX_THR 4
#define DG_ISCALE_MAX_LEVELS 12         /* n + 1 at DG_ISCALE_MAX_SIDE */
#define DG_ISCALE_MAX_SIDE 2048         /* H, W */
typedef struct dg_iscale_spec {
  int speed_u, speed_v;                 /* input channels of the speed channel, or -1, -1: none */
  int nthr;                             /* 1 .. DG_ISCALE_MAX_THR */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];   /* per input channel, finite */
  float thr[DG_HIST_MAX_OUT][DG_ISCALE_MAX_THR];     /* per output channel, the first nthr finite */
} dg_iscale_spec;
int dg_iscale_levels(int H, int W);
int64_t dg_iscale_bound(int H, int W);
size_t dg_iscale_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_iscale_spec* s);
int dg_iscale(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_iscale_spec* s, void* ws, int64_t* sums,
              int64_t* per_field, void* stream);
int dg_iscale_host(const dg_iscale_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* sums);

/* ---- Field-deformation verification (csrc/deform.hip) ------------------------------------------------------------------------
 * By which vector, at which place, does the generated field have to be moved to lie on the real one, and how much error is left
 * once it has been moved: the pyramidal image matcher and the displacement / amplitude split of Keil & Craig (2007, 2009).
 * Fields, series and output values y are those of the fractions skill score above (the same code, csrc/hist_common.h).
 *   quantiser      b = hist_bin(y, lo[j], inv_step[j], 254) in fp32 (the bin rule of the value histograms); q = 0 for the
 *                  underflow code 0 and the NaN code 256, q = b for 1 .. 254, q = 255 for the overflow code 255.  q in 0 .. 255;
 *                  lo is the threshold below which the field counts as empty.  Everything after this is integer.
 *   pyramid        F = levels, 1 .. DG_DEFORM_MAX_LEVELS.  P_0 = q; P_l[i,j] = the SUM of the 2 x 2 block of P_(l-1), zeros
 *                  beyond the grid; level l is ceil(H / 2^l) x ceil(W / 2^l), P_l <= 255 * 4^l <= 65280 (uint16).
 *   matching       "target X, source Y", run in both directions: direction 0 has X = a (real), Y = b (generated), direction 1
 *                  the other way round.  For l = F down to 0, at every level-l pixel p:
 *                    init[p]  = 2 * d_(l+1)[p >> 1]           (0 for l = F; init and Y_l read as 0 outside the level's grid)
 *                    Y'[x]    = Y_l[x + init[x]]              (0 outside the grid)
 *                    cost(p, s) = sum over w in [-2,2]^2 of (X_l[p+w] - Y'[p+w+s])^2,  s = (sy, sx) in [-2,2]^2
 *                    s*       = the s of least cost; of equal costs the first in the order sorted by (sy^2 + sx^2, sy, sx):
 *                               the zero shift wins every tie
 *                    d_l[p]   = s* + init[p + s*]             the composition of backward warps: Y_0[p + d_0[p]] is the morphed
 *                                                             field M (0 where p + d_0[p] is outside the grid)
 *                  |d_0| components <= D = 2 (2^(F+1) - 1) (30 at F = 3, 62 at F = 4).  A cost is <= 25 (255 * 4^l)^2: below
 *                  2^32 for l <= 2, 64 bits for l = 3, 4.
 *   sums           exact integers per (output channel, direction) over all fields:
 *                    disp[(2D+1)^2]   counts of the vector d_0[p] over the pixels with X_0[p] > 0, index (dy+D)(2D+1) + dx+D
 *                    scalars[5]       n_target = #{X_0 > 0}, n_either = #{X_0 > 0 or M > 0}, sse_morphed = sum (X_0 - M)^2,
 *                                     sse_raw = sum (X_0 - Y_0)^2, energy = sum X_0^2
 * A kernel per series quantises every pixel once (uint8), one per level halves the pyramid (uint16), one per level matches both
 * directions of every field: a workgroup owns a 64 x 32 tile, stages X_l (halo 2), Y' (halo 4, one gather through the parent
 * displacement each) and init (halo 2) in LDS; a thread owns one column of 8 pixels and for each of the 25 shifts, in the tie
 * order, sums the squared differences of a row of 5 once per row and slides the 5 rows down its column, keeping the best cost
 * with a strict <.  The last kernel forms M and the sums: the displacement table as an LDS histogram per workgroup, flushed by one
 * 64-bit integer atomic per non-zero bin.  No float after the quantiser, integer atomics only: exact, and two calls on the same
 * data are bit-identical.
 *
 * dg_deform_bound: host-side, 65025 H W, the most one field adds to any sum; 0 when H or W is outside 1 .. DG_DEFORM_MAX_SIDE.
 * dg_deform_ws_bytes: workspace bytes of one call (0 for an invalid descriptor, grid or spec, for T * H * W > 2^31 and for
 *   T * dg_deform_bound > 2^62): per field, output channel and side the pyramid, per direction the displacements of all levels.
 * dg_deform: disp int64 [nout][2][(2D+1)^2] and scalars int64 [nout][2][5] ACCUMULATE (the caller zeroes them and owns their
 *   headroom).  Rejected before any launch: descriptors that differ in T / C / P, P != H*W, levels outside 1 ..
 *   DG_DEFORM_MAX_LEVELS, a non-finite lo / scale / offset, an inv_step that is not finite and > 0, and what dg_deform_ws_bytes
 *   rejects.
 * dg_deform_field: d_0 as int16 [T][nout][2 directions][2 (dy, dx)][H][W] and, unless NULL, M as uint8 [T][nout][2][H][W];
 *   both overwritten.  The same checks and workspace as dg_deform.
 * dg_deform_host / dg_deform_field_host: host-side, the same definition for one field pair, planar fp32 [C][H][W], by the plain
 *   625-term loop per pixel; disp and scalars +=, field int16 [nout][2][2][H][W] and morphed uint8 [nout][2][H][W] (or NULL)
 *   overwritten. */
#define DG_DEFORM_MAX_LEVELS 4
#define DG_DEFORM_MAX_SIDE 2048         /* H, W */
#define DG_DEFORM_SCALARS 5
typedef struct dg_deform_spec {
  int speed_u, speed_v;                 /* input channels of the speed channel, or -1, -1: none */
  int levels;                           /* F: 1 .. DG_DEFORM_MAX_LEVELS */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];   /* per input channel, finite */
  float lo[DG_HIST_MAX_OUT], inv_step[DG_HIST_MAX_OUT];   /* per output channel: finite; finite and > 0 */
} dg_deform_spec;
int64_t dg_deform_bound(int H, int W);
size_t dg_deform_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_deform_spec* s);
int dg_deform(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_deform_spec* s, void* ws, int64_t* disp,
              int64_t* scalars, void* stream);
int dg_deform_field(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_deform_spec* s, void* ws,
                    int16_t* field, uint8_t* morphed, void* stream);
int dg_deform_host(const dg_deform_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* disp, int64_t* scalars);
int dg_deform_field_host(const dg_deform_spec* s, const float* a, const float* b, int C, int H, int W, int16_t* field,
                         uint8_t* morphed);

/* ---- Joint histograms (csrc/joint.hip) -------------------------------------------------------------------------------------
 * Wind roses and real-vs-generated densities: 2-D histograms over one or two series of fields of equal T, C, P, each read in
 * place through the EOF descriptor (NCHW fp32 / bf16, the resident feed's [n, H, W, c] store, the generator's padded NHWC
 * output; a and b may differ in layout and dtype).  Series a is the real fields (or the only series), b the generated ones.
 * The output values are those of the value histograms (the same code, csrc/hist_common.h), one transform for both series,
 * every fp32 operation rounded once, never contracted:
 *   y_c = (x_c * scale[c]) + offset[c]
 *   s   = sqrt(y_u * y_u + y_v * y_v)                       speed_u >= 0: the speed of the pair (u, v)
 * An AXIS is (src: 0 = a, 1 = b; chan; nbins; lo; inv_w).  chan 0 .. C-1 is a component, chan = C the speed, chan = C + 1 the
 * direction.  Component and speed axes use the bin rule of the value histograms (hist_bin): index 0 underflow, 1 .. nbins
 * interior, nbins + 1 overflow, nbins + 2 NaN.  A DIRECTION axis has nbins = nsec sectors in the meteorological convention
 * (where the wind comes from, clockwise from north, sector 0 centred on north); nsec is a multiple of 4 in 4 .. 72, shared by
 * every direction axis of the spec, K = nsec / 4, tan_k[k] = fp32(tan(k pi / (4 K))) for k = 1 .. K-1 rounded once from
 * float64 (tan_k[0] is not read), calm is finite and >= 0.  The direction rule, in this order (no atan2: it is not correctly
 * rounded, so it cannot be part of an exact contract):
 *   1. y_u or y_v NaN                       -> index nsec + 2
 *   2. not (s > calm)                       -> index 0 (calm); index nsec + 1 is never used
 *   3. x = -y_u, y = -y_v, ax = |x|, ay = |y|, swap = ax > ay
 *   4. m = swap ? ay : ax,  M = swap ? ax : ay
 *   5. j = #{k in 1 .. K-1 : m >= fp32(M * tan_k[k])}       one rounded multiply per k
 *   6. q = swap ? 2K - 1 - j : j
 *   7. half sector h = q          if x >= 0 && y > 0
 *                      4K - 1 - q if x > 0 && y <= 0
 *                      4K + q     if x <= 0 && y < 0
 *                      8K - 1 - q if x < 0 && y >= 0
 *   8. sector = ((h + 1) >> 1) mod nsec, index = 1 + sector
 * A PAIR is two axes (X, Y); its table is int64 [nbx + 3][nby + 3], row-major, X first, at most DG_HIST2D_MAX_CELLS cells; a
 * spec holds 1 .. DG_HIST2D_MAX_PAIRS pairs and counts holds their tables concatenated in pair order.  Since every axis uses the
 * 1-D rule, the marginals of a table equal the dg_hist counts of the same axis exactly.
 * Consecutive pairs are packed into groups whose uint32 tables together fit the LDS budget of one workgroup; one group is one
 * launch that reads the input once: every workgroup keeps the group's tables in LDS (ds_add_u32) and adds the non-zero cells
 * to counts with 64-bit integer atomics.  Nothing is summed in floating point: the counts are exact for any T * P and two calls
 * on the same data are bit-identical.
 *
 * dg_hist2d_ws_bytes: workspace bytes of one call; 0 for an invalid call, else a small non-zero value (no workspace is needed).
 * dg_hist2d: ACCUMULATES into counts (the caller zeroes them).  b NULL unless an axis has src 1.  Rejected before any launch
 *   (DG_ERR_BAD_SHAPE; DG_ERR_BAD_DTYPE for a dtype other than fp32 / bf16): a NULL pointer, npairs outside 1 ..
 *   DG_HIST2D_MAX_PAIRS, a table above the cell cap, nbins < 1, a non-finite lo or inv_w or inv_w <= 0, a chan that does not
 *   exist, a speed or direction axis without a speed pair, a direction axis whose nbins != nsec, a bad nsec, a negative or
 *   non-finite calm, src 1 with b NULL, series that differ in T, C or P.
 * dg_hist2d_host_bins: host-side, the same transform and rules for xa, xb fp32 [C][n] (planar; xb may be NULL when no axis has
 *   src 1): bins int32 [npairs][2][n], the X and the Y index of every point under every pair. */
#define DG_HIST2D_MAX_PAIRS 8
#define DG_HIST2D_MAX_CELLS 16384
#define DG_HIST2D_MAX_SECTORS 72
typedef struct dg_hist2d_axis { int src, chan, nbins; float lo, inv_w; } dg_hist2d_axis;
typedef struct dg_hist2d_spec {
  int npairs, speed_u, speed_v, nsec;
  float calm, tan_k[DG_HIST2D_MAX_SECTORS / 4];
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];
  dg_hist2d_axis ax[DG_HIST2D_MAX_PAIRS][2];
} dg_hist2d_spec;
size_t dg_hist2d_ws_bytes(const dg_eof_fields* a, const dg_eof_fields* b, const dg_hist2d_spec* s);
int dg_hist2d(const dg_eof_fields* a, const dg_eof_fields* b, const dg_hist2d_spec* s, void* ws, int64_t* counts, void* stream);
int dg_hist2d_host_bins(const dg_hist2d_spec* s, const float* xa, const float* xb, int C, int64_t n, int32_t* bins);

/* ---- Increment histograms (csrc/increments.hip) -----------------------------------------------------------------------------
 * Is the generated field as intermittent as the real one: the distributions of the spatial increments d_r y = y(x + r) - y(x) per
 * separation r, from which follow the structure functions S_p(r), the flatness S_4 / S_2^2 (3 for a Gaussian, growing towards
 * small r in real wind), the skewness, the scaling exponents and, at r = 1, the gradient distribution.  S_2 is the only one of
 * these the spectrum already determines.  Fields are H x W, read through the EOF descriptor with P = H*W, p = h*W + w; series a
 * (real) is required, series b (generated) is optional, of equal T, C, P with its own layout and dtype (NCHW fp32 / bf16, the
 * resident feed's [n, H, W, c] store, the generator's padded NHWC output).  The output values y are those of the value
 * histograms (the same code, csrc/hist_common.h), every fp32 operation rounded once, never contracted:
 *   y_c = (x_c * scale[c]) + offset[c]
 *   s   = sqrt(y_u * y_u + y_v * y_v)                       speed_u >= 0: appended as output channel C (nout = C + 1)
 * For output channel j and lag r = lag[l]:
 *   direction 0 (along w):  d = fp32(y[t,h,w+r] - y[t,h,w])   for 0 <= w < W - r
 *   direction 1 (along h):  d = fp32(y[t,h+r,w] - y[t,h,w])   for 0 <= h < H - r
 * one correctly rounded fp32 subtraction of the already rounded y (hist_diff), never contracted with the affine.  No wrap-around;
 * a lag >= the extent contributes nothing in that direction and is not an error.
 *   bin     = hist_bin(d, lo[j][l], inv_w[j][l], nbins): index 0 underflow, 1 .. nbins interior, nbins + 1 overflow (+-inf land
 *             in under / overflow), nbins + 2 NaN (a NaN operand gives a NaN d, and so does inf - inf)
 *   counts  int64 [nser][nout][2][nlag][nbins + 3]
 *   finite  int64 [nser][nout][2][nlag]       the number of finite d
 *   moments fp64  [nser][nout][2][nlag][6]    over the finite d, u = (double)d:  sum u, |u|, u^2, u^3, |u|^3, u^4, formed as
 *                                             u2 = u*u, u3 = u2*u, u4 = u2*u2
 * nser is 1 (b NULL) or 2.  All three ACCUMULATE (the caller zeroes them).  A workgroup stages a tile of the transformed values
 * of one output channel in LDS with a halo of the largest lag of the direction it serves (long row segments for direction 0,
 * 64-column strips for direction 1), so both operands of every increment come from LDS; the counts come from uint32 LDS tables
 * (ds_add_u32) flushed with 64-bit integer atomics: exact for any T * P and independent of arrival order.  The moments go through
 * per-workgroup partials summed in a fixed order.  No float atomics: two calls on the same data are bit-identical in all three
 * outputs.  When the tables of a spec do not fit beside the tile, the output channels are cut into groups, one launch each.
 *
 * dg_incr_ws_bytes: workspace bytes of one call (0 for an invalid call).
 * dg_incr: rejected before any launch (DG_ERR_BAD_SHAPE; DG_ERR_BAD_DTYPE for a dtype other than fp32 / bf16): a NULL pointer,
 *   P != H*W, H or W outside 1 .. DG_INCR_MAX_SIDE, series that differ in T, C or P, nlag or nbins out of range, lags unsorted or
 *   out of range, a non-finite lo, inv_w, scale or offset, inv_w <= 0, speed channels that do not exist.
 * dg_incr_host: host-side, the same definition for one field of one series, planar fp32 [C][H][W]; adds (+=) into the slices of
 *   one series: counts [nout][2][nlag][nbins + 3], finite [nout][2][nlag], moments [nout][2][nlag][6]. */
#define DG_INCR_MAX_LAGS 8
#define DG_INCR_MAX_LAG  256
#define DG_INCR_MAX_BINS 512
#define DG_INCR_MAX_SIDE 2048
typedef struct dg_incr_spec {
  int speed_u, speed_v;            /* input channels of the speed channel, or -1, -1: none */
  int nlag, nbins;                 /* 1 .. MAX each */
  int lag[DG_INCR_MAX_LAGS];       /* 1 <= lag <= DG_INCR_MAX_LAG, strictly increasing */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];   /* per input channel, finite */
  float lo[DG_HIST_MAX_OUT][DG_INCR_MAX_LAGS], inv_w[DG_HIST_MAX_OUT][DG_INCR_MAX_LAGS];  /* finite; inv_w > 0 */
} dg_incr_spec;
size_t dg_incr_ws_bytes(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_incr_spec* s);
int dg_incr(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_incr_spec* s, void* ws,
            int64_t* counts, int64_t* finite, double* moments, void* stream);
int dg_incr_host(const dg_incr_spec* s, const float* x, int C, int H, int W, int64_t* counts, int64_t* finite, double* moments);

/* ---- Per-gridpoint histograms (csrc/gridhist.hip) ---------------------------------------------------------------------------
 * The distribution AT a gridpoint: one histogram per pixel and output channel over the fields t, from which follow the maps of
 * local quantiles (P95 / P98 / P99 of wind speed, real against generated), the local QQ line and the local Wasserstein and
 * Kolmogorov-Smirnov distances; the tables are also the input of empirical quantile mapping.  One series a, or two series a
 * (real) and b (generated) of equal T, C, P, each read in place through the EOF descriptor (NCHW fp32 / bf16, the resident
 * feed's [n, H, W, c] store, the generator's padded NHWC output; a and b may differ in layout and dtype).  The spec is the
 * dg_hist_spec of the value histograms, and the output values y and their rows are those of dg_hist bit for bit (hist_affine,
 * hist_speed, hist_bin of csrc/hist_common.h): row 0 underflow, 1 .. nbins interior, nbins + 1 overflow, nbins + 2 NaN.  The only
 * new limit is nbins <= DG_GRIDHIST_MAX_BINS, because the table is per pixel:
 *   counts  int32 [nout][S][nbins + 3][P]     S = 1 (b NULL) or 2 (real, generated); the pixel index fastest
 *   counts[j][s][r][p] += #{t : output channel j of series s at pixel p falls in row r}
 * nout * S * (nbins + 3) * P * 4 bytes: 1.6 GB for nout = 3, S = 2, nbins = 64 on a 1024^2 grid, 26 MB on 128^2.  dg_gridhist
 * ACCUMULATES (the caller zeroes the table and keeps every count below 2^31).  A thread owns its pixels (four consecutive ones
 * of an NCHW plane per 16 / 8-byte load, else one), a wave's pixels are contiguous, and the fields are cut into slices over
 * the workgroups when P alone does not fill the chip; a thread walks its fields in t order, combines a run of equal rows in
 * registers and adds it with one no-return 32-bit integer atomic at agent scope.  Integer adds commute: the counts are exact,
 * do not depend on how the fields were chunked into calls, on layout or on dtype (bf16 inputs are the values read), and two
 * calls on the same data are bit-identical.  No float atomics, no partial tables.
 *
 * dg_gridhist_scan reads a table and Q probabilities q_k (HOST pointer, fp64, 0 < q_k < 1, 1 <= Q <= DG_GRIDHIST_MAX_Q) and writes
 * integers only.  Per (j, s, p), with n = the sum of rows 0 .. nbins + 1 (the finite values):
 *   m = fp64(q_k * fp64(n)) (one rounded product);  k = (int64)ceil(m);  b = the first row whose cumulative count is >= k
 *   ranks  int32 [nout][S][Q][3][P] = (b, cumulative count below row b, counts[b]);  (-1, 0, 0) for n = 0
 * (n >= 1 and 0 < q < 1 give 1 <= k <= n, so counts[b] >= 1).  With S = 2, A_r / B_r the cumulative counts of a / b through row
 * r and na / nb their finite totals:
 *   dist   int64 [nout][2][P]
 *   dist[j][0][p] = sum_{r = 0 .. nbins} g_r |A_r nb - B_r na|,  g_0 = g_nbins = 1, every other g_r = 2
 *   dist[j][1][p] = max_{r = 0 .. nbins + 1} |A_r nb - B_r na|
 * both -1 where na = 0 or nb = 0.  The host derives W1 = (w / 2) dist0 / (na nb) and KS = dist1 / (na nb): underflow mass at lo,
 * interior bin at its centre, overflow at hi.  2 (nbins + 1) n^2 must stay below 2^63: the caller keeps n < 2^26.  One lane per
 * pixel (per four pixels where P % 4 == 0) walks the rows twice (totals, then cumulative counts), plane-wise and coalesced; no
 * atomics, no LDS, trip counts depend on nbins and Q only.
 *
 * dg_gridhist_ws_bytes: workspace bytes of one dg_gridhist call (0 for an invalid descriptor or spec; `paired` != 0: two series).
 * dg_gridhist: b NULL = one series; ws may be NULL (the atomics need no partial state).
 * dg_gridhist_scan: dist NULL when S = 1 (required when S = 2).
 * dg_gridhist_host / dg_gridhist_scan_host: host-side, the same definitions in plain C++: xa, xb planar fp32 [T][C][P] (xb NULL:
 *   one series), counts += as above; the scan with the same arguments on host arrays. */
#define DG_GRIDHIST_MAX_BINS 256
#define DG_GRIDHIST_MAX_Q 16
size_t dg_gridhist_ws_bytes(const dg_eof_fields* a, int paired, const dg_hist_spec* s);
int dg_gridhist(const dg_eof_fields* a, const dg_eof_fields* b, const dg_hist_spec* s, void* ws, int32_t* counts, void* stream);
int dg_gridhist_scan(const int32_t* counts, int nout, int S, int nbins, int P, const double* q, int Q, int32_t* ranks,
                     int64_t* dist, void* stream);
int dg_gridhist_host(const dg_hist_spec* s, const float* xa, const float* xb, int C, int T, int P, int32_t* counts);
int dg_gridhist_scan_host(const int32_t* counts, int nout, int S, int nbins, int P, const double* q, int Q, int32_t* ranks,
                          int64_t* dist);

/* ---- Empirical quantile mapping (csrc/qmap.hip) -----------------------------------------------------------------------------
 * The per-gridpoint bias correction y' = F_real^-1(F_gen(y)) (the bias-correction half of BCSD, the "GAN + QM" baseline), fitted
 * on a paired dg_gridhist table and applied to series of fields read through the EOF descriptor.  Every step is integer arithmetic
 * or one correctly rounded floating-point operation with contraction off, so the device and the host references agree bit for bit.
 *
 * dg_qmap_fit: counts int32 [nout][2][nbins + 3][P] as dg_gridhist writes it (side 0 real = the target, side 1 generated = the
 * source), lo[j] (fp32) and width[j] (fp64, the nominal bin width (hi - lo) / nbins; both HOST pointers, nout entries, lo finite,
 * width > 0) -> nodes fp32 [nout][nbins + 3][P], the pixel index fastest.  Per (j, p), a[r] the generated and b[r] the real row:
 *   n_g = sum_{r = 0 .. nbins + 1} a[r], n_r likewise;  G_k = sum_{r <= k} a[r], B_s = sum_{r <= s} b[r], k, s = 0 .. nbins: the
 *   cumulative counts at the bin edges e_k = lo + k w (row 0 is the underflow mass).
 *   n_g = 0 or n_r = 0: pos_k = k (nothing to calibrate on: the identity).  Otherwise in int64 X = G_k n_r, B'_s = B_s n_g (fewer than
 *   2^26 fields: every product is below 2^52 and converts to fp64 exactly) and
 *     X > B'_nbins:  plo = phi = nbins                                    (the target lies in the real overflow mass)
 *     X <= B'_0:     plo = 0, phi = max{s : B'_s <= X} (0 when there is none)
 *     otherwise:     s = the smallest index in 1 .. nbins with B'_s >= X (so b[s] > 0);
 *                    plo = fp64(s - 1) + fp64(X - B'_{s-1}) / fp64(b[s] n_g)   (one division, one addition)
 *                    phi = max(plo, max{s : B'_s <= X})
 *   pos_k = min(max(fp64(k), plo), phi): where the real CDF is flat at the target its inverse is an interval, and the node takes
 *   the point of it nearest to the edge itself -- the least correction, and a == b gives the identity exactly, empty bins included.
 *   nodes[k]         = fp32(fp64(lo) + pos_k w), k = 0 .. nbins           (one fp64 multiply, one fp64 add, one rounding)
 *   nodes[nbins + 1] = d_lo = nodes[0] - lo                               (fp32)
 *   nodes[nbins + 2] = d_hi = nodes[nbins] - fp32(fp64(lo) + nbins w)     (fp32)
 * One lane owns its pixel (four pixels, with 16-byte row accesses, where P % 4 == 0 and the arrays are 16-byte aligned): a first walk
 * for n_g and n_r, then one merge walk in which k, s and the phi pointer only advance.  No LDS, no atomics.
 *
 * dg_qmap_apply: the series x (every layout and dtype dg_gridhist takes), the dg_hist_spec the table was made with (the checks of
 * dg_gridhist) and nodes -> out fp32 [T][nout][P], planar.  Per output value y of the spec (hist_affine, hist_speed), with t and the row
 * r exactly as hist_bin makes them:
 *   NaN row: the quiet NaN 0x7fc00000;   r = 0: y + d_lo;   r = nbins + 1: y + d_hi   (beyond the calibrated range a constant shift)
 *   interior, k = r - 1:  f = t - (float)k;  dm = nodes[k + 1] - nodes[k];  out = nodes[k] + f dm   (three rounded fp32 operations)
 * A workgroup stages the transfer functions of 64 consecutive pixels of one output channel in LDS as [node][pixel] ((nbins + 3) * 256
 * bytes; a lane's reads hit bank pixel mod 32, distinct within its group of 32 lanes) and its waves stream the fields of its slice past them; the fields are cut into
 * slices over blockIdx.y when P alone does not fill the chip.  out is overwritten, two calls are bit-identical, and the result
 * does not depend on how the fields were chunked into calls.
 *
 * dg_qmap_fit_host / dg_qmap_apply_host: host-side, the same definitions in plain C++ on host arrays; x planar fp32 [T][C][P].
 * Status codes as dg_gridhist: DG_ERR_BAD_SHAPE for a NULL pointer, nout, nbins, P, T or a spec out of range, DG_ERR_BAD_DTYPE for
 * a dtype other than fp32 / bf16; nothing is launched then. */
int dg_qmap_fit(const int32_t* counts, int nout, int nbins, int P, const float* lo, const double* width, float* nodes, void* stream);
int dg_qmap_apply(const dg_eof_fields* x, const dg_hist_spec* s, const float* nodes, float* out, void* stream);
int dg_qmap_fit_host(const int32_t* counts, int nout, int nbins, int P, const float* lo, const double* width, float* nodes);
int dg_qmap_apply_host(const dg_hist_spec* s, const float* x, int C, int T, int P, const float* nodes, float* out);

/* ---- Temporal diagnostics (csrc/temporal.hip) -------------------------------------------------------------------------------
 * Every other diagnostic treats the fields of a series as an unordered sample; this one looks along the time axis of one series:
 * how long a gridpoint stays above / below a threshold (spell durations), how fast it changes (ramps y(t) - y(t - tau)) and how
 * persistent it is (lag autocorrelation).  A SERIES is a sequence of fields in time order.  Series a (real) is required, series b
 * (generated) is optional, of equal T, C, P, each read in place through the EOF descriptor (NCHW fp32 / bf16, the resident feed's
 * [n, H, W, c] store, the generator's padded NHWC output; a and b may differ in layout and dtype).  S = 1 (b NULL) or 2.  The
 * output values y are those of the value histograms bit for bit (hist_affine, hist_speed of csrc/hist_common.h, the speed
 * appended as output channel C: nout = C + 1 with speed_u >= 0, else C).
 * Time is absolute: a call carries t0, the number of fields added before it, and its fields are the times t0 .. t0 + T - 1.
 * Everything below ACCUMULATES into caller-owned device arrays (zeroed by the caller before the first call); the pixel index is
 * fastest wherever P appears.
 *
 * Spells.  Condition k of output channel j: y > thr[j][k] (below[k] = 0) or y < thr[j][k] (below[k] = 1), fp32 compares: false
 * for NaN and for equality.  A spell of (s, j, k, p) is a maximal run of consecutive times at which the condition holds; it
 * completes at the first time at which the condition fails.
 *   open     int32 [S][nout][nthr][P]       the length of the run still open after the last field added (carried state)
 *   spells   int64 [S][nout][nthr][ndur]    spells[..][min(len, ndur) - 1] += 1 per completed spell, pooled over the pixels
 *   spellmap int32 [S][nout][nthr][3][P]    row 0: completed spells; row 1: the total time in completed spells; row 2: the
 *                                           longest run seen, open runs included
 * A run still open after the last field is in no row of spells (it is right-censored; the caller reads it from open).  A run that
 * starts at time 0 is counted like any other although its true start is unknown: it is LEFT-CENSORED.
 *
 * Ramps.  For tau = lag[l] and t - tau >= 0: d = hist_diff(y[t], y[t - tau]), one rounded fp32 subtraction of the rounded y.
 *   ramps    int64 [S][nout][nlag][nbins + 3]   ramps[..][hist_bin(d, lo[j][l], inv_w[j][l], nbins)] += 1, pooled over the pixels
 * with the rows of dg_hist (0 underflow, 1 .. nbins interior, nbins + 1 overflow, nbins + 2 NaN: a NaN operand, or inf - inf).
 *
 * Persistence.  Per (s, j, p), never contracted, every sum in fp64 added in t order:
 *   accnt    int32 [S][nout][1 + nlag][P]       row 0: n = #{t : y[t] finite};  row 1 + l: m_l = #{t : y[t], y[t - tau_l] finite}
 *   acsum    fp64  [S][nout][2 + 2 nlag][P]     row 0: s1 = sum (double)y;  row 1: s2 = sum (double)y * (double)y  (finite y);
 *                                               row 2 + 2l: c_l = sum (double)y[t] * (double)y[t - tau_l]  (the product of two
 *                                               fp32 is exact in fp64);  row 3 + 2l: e_l = sum ((double)y[t] + (double)y[t - tau_l])
 *                                               (both over the t counted by m_l)
 *   tail     fp32  [S][nout][R][P], R = lag[nlag - 1]: tail[..][t mod R] = y at time t for the last R times (carried state;
 *                                               absent -- may be NULL -- when nlag = 0)
 * The host derives mu = s1 / n and r_l = (c_l / m_l - mu e_l / m_l + mu^2) / (s2 / n - mu^2).
 *
 * The chunking contract: every output, the bits of the fp64 sums and the carried state included, is the same however the series
 * was cut into calls (calls of one field and calls shorter than the largest lag included), and does not depend on layout or
 * dtype (bf16 inputs are the values read); two runs on the same data are bit-identical.  The fields of a call are therefore NOT
 * cut into time slices: a thread owns its pixels (four consecutive ones of an NCHW plane per 16 / 8-byte load on large grids,
 * else one) of one output channel of one series and walks the call's fields in t order with its open runs, counts and fp64 sums
 * in registers; y[t - tau] is recomputed from field t - tau of the same call (a second read, served by the caches) or, for
 * t - tau < t0, taken from tail.  The pooled tables go through uint32 LDS tables flushed with 64-bit integer atomics.  Integer
 * atomics only, no float atomics, no loop whose trip count depends on data.
 *
 * dg_temporal_ws_bytes: workspace bytes of one call (0 for an invalid call, else a small non-zero value: no workspace is needed).
 * dg_temporal: ws may be NULL.  open, spells, spellmap may be NULL when nthr = 0; tail, ramps when nlag = 0.  Rejected before any
 *   launch (DG_ERR_BAD_SHAPE; DG_ERR_BAD_DTYPE for a dtype other than fp32 / bf16): a NULL pointer that is needed, series that
 *   differ in T, C or P, nthr, ndur, nlag or nbins out of range, nthr = nlag = 0, a below that is not 0 or 1, lags unsorted or
 *   out of range, a non-finite thr, lo, inv_w, scale or offset, inv_w <= 0, speed channels that do not exist, t0 < 0,
 *   t0 + T >= 2^31.
 * dg_temporal_host: host-side, the same definition in plain C++ for ONE series, planar fp32 [T][C][P], with the same t0 and the
 *   state and output arrays of one series (the [S] dimension dropped). */
#define DG_TEMPORAL_MAX_THR 4
#define DG_TEMPORAL_MAX_DUR 256
#define DG_TEMPORAL_MAX_LAGS 4
#define DG_TEMPORAL_MAX_LAG 24
#define DG_TEMPORAL_MAX_BINS 512
typedef struct dg_temporal_spec {
  int speed_u, speed_v;                    /* input channels of the speed channel, or -1, -1: none */
  int nthr, ndur, nlag, nbins;             /* 0 .. MAX_THR, 1 .. MAX_DUR, 0 .. MAX_LAGS, 1 .. MAX_BINS; nthr + nlag >= 1 */
  int below[DG_TEMPORAL_MAX_THR];          /* 0: y > thr; 1: y < thr */
  int lag[DG_TEMPORAL_MAX_LAGS];           /* 1 <= lag <= DG_TEMPORAL_MAX_LAG, strictly increasing */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];                   /* per input channel, finite */
  float thr[DG_HIST_MAX_OUT][DG_TEMPORAL_MAX_THR];                   /* finite */
  float lo[DG_HIST_MAX_OUT][DG_TEMPORAL_MAX_LAGS], inv_w[DG_HIST_MAX_OUT][DG_TEMPORAL_MAX_LAGS];   /* finite; inv_w > 0 */
} dg_temporal_spec;
size_t dg_temporal_ws_bytes(const dg_eof_fields* a, const dg_eof_fields* b, const dg_temporal_spec* s);
int dg_temporal(const dg_eof_fields* a, const dg_eof_fields* b, const dg_temporal_spec* s, int64_t t0, void* ws, int32_t* open,
                float* tail, int64_t* spells, int32_t* spellmap, int64_t* ramps, double* acsum, int32_t* accnt, void* stream);
int dg_temporal_host(const dg_temporal_spec* s, const float* x, int C, int T, int P, int64_t t0, int32_t* open, float* tail,
                     int64_t* spells, int32_t* spellmap, int64_t* ramps, double* acsum, int32_t* accnt);

/* ---- Exceedance objects (csrc/objects.hip) ----------------------------------------------------------------------------------
 * Every other diagnostic treats a field as a bag of pixels or of Fourier modes; this one knows that the pixels above a threshold
 * form things: a gust front, a lee jet, a convective cell, each with an area, a mass, a peak and a place.  From the records follow
 * object counts and size distributions, per-object hits / misses / false alarms and the SAL score (Wernli et al. 2008), all formed
 * on the host.  Fields are H x W, read through the EOF descriptor with P = H*W, p = h*W + w; series a (real) is required, series b
 * (generated) is optional, of equal T, C, P with its own layout and dtype (NCHW fp32 / bf16, the resident feed's [n, H, W, c] store,
 * the generator's padded NHWC output).  The output values y are those of the value histograms and of the fractions skill score
 * (hist_affine, hist_speed of csrc/hist_common.h): C components plus the optional speed channel appended last (nout = C + 1).
 * For output channel j and threshold k:
 *   mask        I[t,p] = (y > thr[j][k]), an fp32 compare: NaN is false, +inf is true, equality is false
 *   object      a connected component of the mask; connectivity 4 joins edge neighbours, 8 adds the corner neighbours
 *   root        the smallest linear index h*W + w among the object's pixels: the object's identity within its plane
 *   intensity   q = clamp(rint(t), 0, 2^24 - 1), t = fp32(y * inv_quantum): one fp32 multiply, round to nearest even;
 *               t >= 16777215.f gives 2^24 - 1, a negative t gives 0 (a NaN y is never in a mask)
 * The RECORD of an object is one row of DG_OBJ_COLS = 12 int64:
 *   [plane, root, area, overlap, mass, sum_qh, sum_qw, qmax, h0, h1, w0, w1]
 *   plane     ((t*2 + side)*nout + j)*nthr + k; t the field's index within the call, side 0 = a (real), 1 = b (generated)
 *   area      the pixel count
 *   overlap   the number of the object's pixels that are also set in the other side's mask of the same (t, j, k); 0 when b is NULL
 *   mass      sum q;  sum_qh = sum q*h;  sum_qw = sum q*w;  qmax = max q
 *   h0 .. w1  the bounding box, inclusive
 * H, W <= DG_OBJ_MAX_SIDE keeps sum q*h below 2^24 * 2^11 * 2^22 = 2^57.  Everything is integer after the compare and the rounding:
 * the records are exact, do not depend on the order of arrival, on layout or on dtype (bf16 inputs are the values read), and two
 * calls on the same data agree in every bit (up to the order of the rows).
 *
 * Device algorithm (labels and slot ids are int32 planes of the workspace, 8 bytes per pixel and plane):
 *   init     one wave per row: the masks of all (j, k) as wave ballots; a set pixel's first label is the index of the first pixel
 *            of its horizontal run (from the ballot, with a wave-uniform carry across 64-pixel chunks), a clear pixel's is -1
 *   merge    lock-free union-find: a set pixel joins its run with the set neighbours of the row above (N; NW and NE for 8) --
 *            find both roots, atomicMin the smaller into the larger root's label, continue from the value the atomic returns
 *   flatten  label[p] = find(p); links only ever point to smaller member indices, so the root is the smallest index
 *   slots    every root draws a record slot from a counter (one atomic per wave), bumps per_plane, writes plane / root and the
 *            initial record and stores its slot id in the second int32 plane; slots at or beyond capacity are counted only
 *   stats    every set pixel adds to its object's record with 64-bit integer atomics (add, min, max); consecutive lanes of a
 *            wave that share a root combine first, so a row segment of an object costs one set of atomics per 64 pixels
 * No lane, wave or workgroup ever waits for a value another one writes; every loop of find and union walks strictly decreasing
 * indices and carries a hard cap of P steps, at which it sets an error word and leaves: dg_objects then returns DG_ERR_LAUNCH.
 *
 * dg_objects_ws_bytes: workspace bytes of one call, sized for both sides (0 for an invalid descriptor, grid or spec, or when
 *   T*2*nout*nthr * ceil(P/2), the most objects a call can hold, reaches 2^31: cut the fields into more calls).
 * dg_objects: count (device int64[1]) receives the true number of objects of the call, also when it exceeds capacity; per_plane
 *   (device int64 [T*2*nout*nthr]) receives the exact object count of every plane, always (the side-1 entries are zero when b is
 *   NULL); table is int64 [capacity][12] and holds every record when count <= capacity, in unspecified row order ((plane, root) is
 *   a unique key); its content is unspecified when count > capacity, and nothing is written past capacity rows.  The call waits
 *   for the stream once, to read the error word.  Rejected before any launch (DG_ERR_BAD_SHAPE; DG_ERR_BAD_DTYPE for a dtype
 *   other than fp32 / bf16): a NULL pointer that is needed (table may be NULL when capacity is 0), descriptors that differ in
 *   T, C or P, P != H*W, a side above DG_OBJ_MAX_SIDE, connectivity not 4 or 8, nthr outside 1 .. DG_OBJ_MAX_THR, a non-finite
 *   thr, scale, offset or inv_quantum, inv_quantum <= 0, speed channels that do not exist, capacity < 0.
 * dg_objects_host: host-side, the same definition for one field (b NULL) or one field pair, planar fp32 [C][H][W], by a plain
 *   flood fill; t = 0 in plane; rows sorted by (plane, root); count, per_plane ([2*nout*nthr]) and capacity as above. */
#define DG_OBJ_MAX_SIDE 2048
#define DG_OBJ_MAX_THR 4
#define DG_OBJ_COLS 12
typedef struct dg_objects_spec {
  int speed_u, speed_v;                 /* input channels of the speed channel, or -1, -1: none */
  int nthr;                             /* 1 .. DG_OBJ_MAX_THR */
  int connectivity;                     /* 4 or 8 */
  float inv_quantum;                    /* finite, > 0: q = rint(y * inv_quantum) */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];   /* per input channel, finite */
  float thr[DG_HIST_MAX_OUT][DG_OBJ_MAX_THR];        /* per output channel, the first nthr finite */
} dg_objects_spec;
size_t dg_objects_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_objects_spec* s);
int dg_objects(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_objects_spec* s, void* ws, int64_t* table,
               int64_t capacity, int64_t* count, int64_t* per_plane, void* stream);
int dg_objects_host(const dg_objects_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* table, int64_t capacity,
                    int64_t* count, int64_t* per_plane);

/* ---- Distance maps (csrc/distmap.hip) ---------------------------------------------------------------------------------------
 * How far from a real exceedance does the generator put its exceedances, in pixels?  The exact Euclidean distance transform (EDT)
 * of the exceedance masks, and from it the distance measures of binary fields: the mean error distance (MED) in both directions
 * (generated -> real: false alarms; real -> generated: misses), the Hausdorff distance, the ring counts behind the partial
 * Hausdorff distance, and the sums of Baddeley's Delta.  Fields, layouts, dtypes, the output values y and the masks
 * y > thr[j][k] (NaN never set) are those of the exceedance objects above; side 0 = a (real, mask A), side 1 = b (generated, B).
 *   d2(x)     int32: the squared Euclidean distance in pixels from x to the nearest set pixel of the plane; 0 on the mask;
 *             DG_DIST_FAR = 2^30 everywhere when the mask is empty
 *   ring(d2)  the smallest integer r with d2 <= r*r (the distance rounded up), in integers
 *   dq(d2)    floor(sqrt(d2 * 2^20)): the distance in units of 2^-10 px, exact in 64-bit integers (a sqrt is a first guess only,
 *             corrected by integer multiplies); dq(25) = 5120
 *   w(x)      min(dq(d2(x)), cutoff * 1024), and cutoff * 1024 where d2 is FAR; cutoff in 1 .. DG_DIST_MAX_CUTOFF pixels
 * The RECORD of a field pair (t, j, k) is one row of DG_DIST_COLS = 11 int64:
 *   [n_a, n_b, n_ab, sum_dq_b2a, sum_d2_b2a, max_d2_b2a, sum_dq_a2b, sum_d2_a2b, max_d2_a2b, bad1, bad2]
 *   n_a, n_b, n_ab   pixels in A, in B, in both
 *   *_b2a            sum / max over x in B of dq(d2_A(x)), d2_A(x);  *_a2b: over x in A of dq(d2_B(x)), d2_B(x)
 *   bad1, bad2       sum over ALL pixels of |w_A - w_B| and of (w_A - w_B)^2
 * Columns 3 .. 8 are all -1 unless n_a > 0 and n_b > 0; bad1 and bad2 are always defined.  With H, W <= DG_DIST_MAX_SIDE and
 * cutoff <= 512, bad2 <= 2^22 * 2^38 = 2^60 and the other sums stay below 2^45: a record cannot overflow (records are per field
 * and never summed on the device).
 * The RING TABLE is int64 [nout][nthr][2][nring + 2], accumulated (the caller zeroes it): direction 0 counts the pixels of B by
 * ring(d2_A), direction 1 the pixels of A by ring(d2_B); bin r < nring holds ring r (bin 0: the overlap), bin nring the pixels
 * with ring >= nring, bin nring + 1 the pixels of a field whose other side is empty.
 * Everything is integer after the compare: results are exact, do not depend on the order of arrival, on layout or on dtype (bf16
 * inputs are the values read), and agree in every bit from run to run.
 *
 * Device algorithm (the workspace holds one uint16 per plane pixel and nothing else):
 *   columns   one thread per column of a (t, side): down the column, g = the distance to the nearest set pixel above (0xFFFF:
 *             none), for all (j, k) at once; then one thread per column of a plane: up, g lowered to the distance to the nearest
 *             set pixel below
 *   rows      one workgroup per row of a (t, j, k), both sides: g^2 in LDS; each pixel scans outward, best = min(best, D^2 +
 *             g^2[w +- D]) while D^2 < best -- exact, since no candidate with D^2 >= best can win; a row without a finite g
 *             belongs to an empty plane and is not scanned; ring, dq and w of both sides; wave reductions, one set of 64-bit
 *             integer atomics per wave into the record, the ring bins through an LDS table
 *   finalize  one thread per record writes the -1 columns
 *
 * dg_distmap_ws_bytes: workspace bytes of one call, sized for both sides: T*2*nout*nthr*P*2 (0 for anything invalid).
 * dg_distmap: records int64 [T][nout][nthr][11], overwritten, may be NULL; rings accumulates, may be NULL; d2 int32
 *   [T][2][nout][nthr][P], may be NULL.  When b is NULL (one series: the EDT alone) d2 must be given, records and rings must be
 *   NULL, and the side-1 planes of d2 are left untouched.  Asynchronous on the stream.  Rejected before any launch
 *   (DG_ERR_BAD_ARG; DG_ERR_BAD_DTYPE for a dtype other than fp32 / bf16): a NULL pointer that is needed, descriptors that differ
 *   in T, C or P, P != H*W, a side above DG_DIST_MAX_SIDE, nthr, nring or cutoff out of range, a non-finite thr, scale or offset,
 *   speed channels that do not exist, nothing to compute (b given and records, rings, d2 all NULL).
 * dg_distmap_host: host-side, the same definition for one field (b NULL) or one field pair, planar fp32 [C][H][W], in plain C++:
 *   records [nout][nthr][11], rings as above (accumulated), d2 [2][nout][nthr][P]; the same rules for NULL.
 * dg_distmap_host_scalars: host-side, ring, dq and w of one d2 in 0 .. DG_DIST_FAR: the integer definitions above on their own. */
#define DG_DIST_MAX_SIDE 2048
#define DG_DIST_MAX_THR 4
#define DG_DIST_MAX_RINGS 128
#define DG_DIST_MAX_CUTOFF 512
#define DG_DIST_COLS 11
#define DG_DIST_FAR (1 << 30)
typedef struct dg_distmap_spec {
  int speed_u, speed_v;                 /* input channels of the speed channel, or -1, -1: none */
  int nthr;                             /* 1 .. DG_DIST_MAX_THR */
  int nring;                            /* 1 .. DG_DIST_MAX_RINGS */
  int cutoff;                           /* 1 .. DG_DIST_MAX_CUTOFF pixels: the cap of Baddeley's w */
  float scale[DG_EOF_MAX_C], offset[DG_EOF_MAX_C];   /* per input channel, finite */
  float thr[DG_HIST_MAX_OUT][DG_DIST_MAX_THR];       /* per output channel, the first nthr finite */
} dg_distmap_spec;
size_t dg_distmap_ws_bytes(const dg_eof_fields* a, int H, int W, const dg_distmap_spec* s);
int dg_distmap(const dg_eof_fields* a, const dg_eof_fields* b, int H, int W, const dg_distmap_spec* s, void* ws, int64_t* records,
               int64_t* rings, int32_t* d2, void* stream);
int dg_distmap_host(const dg_distmap_spec* s, const float* a, const float* b, int C, int H, int W, int64_t* records, int64_t* rings,
                    int32_t* d2);
int dg_distmap_host_scalars(int32_t d2, int cutoff, int32_t* ring, int64_t* dq, int64_t* w);

#ifdef __cplusplus
}
#endif
#endif /* DOWNGAN_HIP_H */
