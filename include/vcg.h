/*
 * vcg.h — C ABI of libvcg.so, the MI355X (gfx950) native kernels behind the
 * VAE-CycleGAN training step.
 *
 * The reference (Baverne/VAE-CYCLEGAN-Implementation) has no FFI of its own:
 * every op below replaces a torch call site inside Networks.py / Losses.py.
 * The citation after each entry point is the reference line it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch's caching
 *     allocator); the library never allocates, frees or synchronises;
 *   - activations are fp32 NHWC with a channel pitch that is a multiple of 4
 *     (3-channel images are stored with pitch 4, pad channel == 0);
 *   - conv weights live in the reference's OIHW layout (state_dict parity) and
 *     are repacked once per optimizer step into the GEMM layout Wf[K][Cout];
 *   - all launches go to `stream` (a hipStream_t passed as void*);
 *   - return 0 on success, negative on error; vcg_last_error() has the text.
 *     Nothing throws across this boundary.
 */
#ifndef VCG_H
#define VCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VCG_ABI_VERSION 6   /* 6 (round 4): vcg_amax_valid, the explicit-argument forms vcg_*_h.  5: vcg_conv_reads_wf, cd[VCG_CD_PACK_FLAGS].  4: vcg_amax_measure.  3 (round 3): packed weights and kept forward state carry fp16 x 2 planes + amax
                               words (sizes changed); vcg_amax_hint / vcg_amax_last.  round 2: vcg_adam_step takes 1 - beta; vcg_conv_fwd_in,
                               vcg_conv_wgrad_saved, input transforms, profiling */

/* Operand magnitudes (round 3) ------------------------------------------------
 * The MFMA kernels compute fp32 products as three fp16 MFMAs: every operand is scaled by a power of two taken from the
 * largest magnitude ("amax") of its tensor and split into two fp16 pieces (csrc/vcg_common.h).  An entry point that reads
 * a tensor whose amax it does not know measures it with one pass over the tensor.  The entry points that WRITE activations
 * and gradients (vcg_in_apply, vcg_in_bwd, vcg_act_bwd) publish the amax of what they wrote as a by-product:
 *   vcg_amax_last()        handle of the amax of the tensor the last such call on this thread wrote (0: none); reading resets it;
 *   vcg_amax_hint(x, dy)   handles for the x / dy operands of the NEXT vcg_conv_fwd / _fwd_in / _dgrad / _wgrad(_saved) call
 *                          on this thread (0 = unknown: measured); consumed by that call.
 * A handle names device-side state of the library's code object; it stays valid for the next 10 239 amax generations on the
 * device (16384 slots less a margin of 6144, csrc/misc.hip; every library call that measures or publishes an amax takes one, a
 * training step ~1 500) and is refused — the tensor is measured — from the 10 240th on.  Passing a handle that belongs to
 * another tensor scales that operand wrongly: hand over only what vcg_amax_last returned for exactly that tensor. */
void vcg_amax_hint(uint64_t x_amax, uint64_t dy_amax);
uint64_t vcg_amax_last(void);
/* Measure a tensor nobody published an amax for (n floats at t, 16-byte aligned), once, on `stream`: the handle serves every
 * later call that reads the tensor on a stream ordered after this one (a forward and the weight gradient that re-reads x; the
 * weight and data gradient of one dy) instead of each of them measuring it again.  0: no slot on this device (callers pass 0 on:
 * the consumers measure). */
uint64_t vcg_amax_measure(const float* t, size_t n, void* stream);
/* 1 while `handle` would still be honoured on the current device, 0 once it is too old (or is not a handle): a caller that keeps
 * handles across many calls (ops.py keeps one per tensor object) asks before handing one on and measures again — refreshing what it
 * keeps — instead of carrying a handle every consumer refuses.  A handle is honoured while its slot is >= 6144 generations from
 * reuse: the check runs when a kernel is enqueued, the kernel reads the slot up to one training step (~1 500 generations) later. */
int vcg_amax_valid(uint64_t handle);
/* A handle describes the tensor's CONTENTS at the time it was published: a caller that lets anything write into the tensor
 * afterwards (in-place ops, buffer reuse) must drop the handle (ops.py keys it on torch's version counter and the data pointer).
 *
 * Explicit-argument forms (ABI v6) — the same calls with the operand handles as arguments and the handle of what the call wrote
 * returned through a pointer, for callers that do not want per-thread state between two calls; vcg_amax_hint / vcg_amax_last
 * remain as the shim they are built on:
 *   vcg_conv_fwd_in_h(..., x_amax, stream)             == vcg_amax_hint(x_amax, 0);  vcg_conv_fwd_in(...)
 *   vcg_conv_dgrad_h(..., dy_amax, stream)             == vcg_amax_hint(0, dy_amax); vcg_conv_dgrad(...)
 *   vcg_conv_wgrad_saved_h(..., x_amax, dy_amax, stream)
 *   vcg_in_apply_h / vcg_in_bwd_h / vcg_act_bwd_h(..., &amax_of_what_was_written, stream)   (pointer may be NULL)
 * declared next to their base forms below. */

/* conv descriptor: int32[16] ------------------------------------------------ */
enum {
  VCG_CD_N = 0,      /* batch */
  VCG_CD_H = 1,      /* physical input height */
  VCG_CD_W = 2,      /* physical input width */
  VCG_CD_CIN = 3,    /* physical input channel pitch (multiple of 4) */
  VCG_CD_COUT = 4,   /* physical output channel pitch (multiple of 4) */
  VCG_CD_KH = 5,
  VCG_CD_KW = 6,
  VCG_CD_STRIDE = 7, /* 1 or 2 */
  VCG_CD_PAD = 8,
  VCG_CD_REFLECT = 9, /* 1 = padding_mode='reflect', 0 = zeros */
  VCG_CD_UPS = 10,   /* 1, or 2 = nn.PixelUnshuffle(2) folded into the gather */
  VCG_CD_ACT = 11,   /* epilogue activation: VCG_ACT_* */
  VCG_CD_CIN_LOGICAL = 12, /* channels of the physical input that carry data (3 for images) */
  VCG_CD_COUT_LOGICAL = 13,
  VCG_CD_PACK_FLAGS = 14,  /* vcg_pack_weight only: bit 0 = leave the fp32 Wf block out (vcg_conv_reads_wf); 0 everywhere else */
  VCG_CD_LEN = 16
};

enum { VCG_ACT_NONE = 0, VCG_ACT_RELU = 1, VCG_ACT_LEAKY02 = 2, VCG_ACT_TANH = 3, VCG_ACT_SIGMOID = 4 };   /* CaSb's choices, Networks.py:62-73 */

int vcg_abi_version(void);
const char* vcg_last_error(void);

/* Diagnostic (bench.py's `roofline` object; the training path never enables it): while enabled, every MFMA kernel launch
   is bracketed by HIP events on its launch stream.  vcg_profile_read WAITS for those events (the one call of this library
   that synchronises) and writes one line per device kernel: name \t launches \t total ms \t executed FLOPs
   (fp32-equivalent: 2*M*N*K of the GEMM the launch ran); returns the bytes written — or, with buf NULL, the bytes a
   following call will need (the table is kept until it has been copied out). */
int vcg_profile_enable(int on);
long vcg_profile_read(char* buf, size_t cap);

/* layout ------------------------------------------------------------------- */
/* x.to(channels-last); images get channel pitch P (pad channels zeroed).     */
int vcg_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W, int P, void* stream);
int vcg_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, int P, void* stream);
int vcg_fill(float* dst, float value, size_t n, void* stream);

/* nn.Conv2d(padding_mode='reflect') — Networks.py:60,87,101,104,122,136,145 -- */
/* OIHW -> the packed buffer every conv entry point below takes as `wf` (repacked once per optimizer step):
     Wf[K][Cout]          K ordered (kh,kw,i,j,c), so PixelUnshuffle (Networks.py:86) needs no data movement;
                          the B operand of the data-gradient and weight-gradient GEMMs
     U, Ud[16][..]        3x3 / stride-1 layers: the Winograd F(2x2,3x3) transforms G g G^T of the kernel (forward,
                          [xi][Cout][K]) and of the flipped kernel (data gradient, [xi][K][Cout]), ALREADY SCALED AND SPLIT into
                          the two fp16 pieces the GEMMs multiply with ("blocked planes": 128 bytes per row and 32-wide block)
     Wk, Wkd              7x7 layers with <= 4 channels on one side: kw folded into the GEMM's N (forward / data gradient)
     WFT, WFD planes      other layers with >= 64 output channels: the transpose of Wf (forward) and its rows per tap (data
                          gradient), pre-split the same way for the direct split-operand kernels
   vcg_pack_weight_floats: floats the caller must provide for `wf` (spatial fields of cd are ignored).
   vcg_conv_reads_wf(cd): 1 if vcg_conv_fwd / _fwd_in / _dgrad at THIS geometry (N, H, W count) read the fp32 Wf block of the
     pack — the thin layers, tiles the split-operand kernels do not take, maps Winograd cannot take — 0 if every direction runs
     from the pre-split planes.  A caller whose layer answers 0 for every geometry it is used at may set cd[VCG_CD_PACK_FLAGS] = 1
     in the descriptor it hands to vcg_pack_weight: the Wf block is then not written (round 3: 0.6 ms and 1 GB per training step
     for the D / R / U layers, whose Wf nothing reads).  Reading a Wf that was left out is undefined: ask again when the geometry
     changes, and repack in full if the answer does. */
size_t vcg_pack_weight_floats(const int32_t* cd);
int vcg_conv_reads_wf(const int32_t* cd);
int vcg_pack_weight(const float* w_oihw, float* wf, const int32_t* cd, void* stream);
/* y = act(conv(x) + bias).  fp32 in, fp32 out, fp32 accumulate; the GEMMs run on the 16-bit matrix pipe
   (v_mfma_f32_{32x32x16,16x16x32}_f16) with every fp32 operand scaled by a power of two and split into two fp16 pieces, three
   products per multiply-add (fp32-level rounding, csrc/vcg_common.h); thin layers use v_mfma_f32_32x32x2_f32.
   3x3 / stride-1 layers go through Winograd F(2x2,3x3) (16 batched GEMMs, V and M in `ws`); layers with few
   output tiles slice K across workgroups into fp32 slabs in `ws` (vcg_conv_fwd_workspace bytes, may be 0). */
size_t vcg_conv_fwd_workspace(const int32_t* cd);
int vcg_conv_fwd(const float* x, const float* wf, const float* bias, float* y,
                 const int32_t* cd, void* ws, size_t ws_bytes, void* stream);

/* The same convolution when an InstanceNorm follows it (CaSb with norm=True, /root/reference/Networks.py:93-95): y as
   above AND mean / rstd (N x Cout each) of y over its pixels, biased variance, rstd = 1 / sqrt(var + eps) — what
   vcg_in_stats(y) returns.  Where the conv's launch plan allows (Winograd output transform; direct split-operand tiles
   with Ho*Wo % 128 == 0; the LDS-slab pixel blocks) the statistics' partial sums (in double) are written by the conv's own
   epilogue, so y is not read again; otherwise the separate reduction pass runs.  mean == rstd == NULL: no statistics,
   the plain forward.  `ws`: vcg_conv_fwd_in_workspace(cd) bytes (vcg_conv_fwd_workspace when mean is NULL).
   `saved` (may be NULL): vcg_conv_saved_floats(cd) floats in which the call leaves forward state that the weight gradient
   of the same (x, cd) can reuse instead of recomputing it — vcg_conv_wgrad_saved below; 0 floats: nothing to keep. */
size_t vcg_conv_fwd_in_workspace(const int32_t* cd);
size_t vcg_conv_saved_floats(const int32_t* cd);
int vcg_conv_fwd_in(const float* x, const float* wf, const float* bias, float* y, float* mean, float* rstd, float eps,
                    float* saved, const int32_t* cd, void* ws, size_t ws_bytes, void* stream);
int vcg_conv_fwd_in_h(const float* x, const float* wf, const float* bias, float* y, float* mean, float* rstd, float eps,
                      float* saved, const int32_t* cd, void* ws, size_t ws_bytes, uint64_t x_amax, void* stream);
/* The fused Conv + InstanceNorm + activation hand-off (round 4; /root/reference/Networks.py:93-95, 110-115: a block's
   InstanceNorm output feeds the next block's conv).  `t_prev` is the RAW output of the previous block's conv — what
   vcg_conv_fwd_in left in y, with its statistics pre_mean / pre_rstd ([N][Cin]) — and this conv's input gather computes
   pre_act((t_prev - mean) * rstd) on the way in: the normalised tensor is never written or read (vcg_in_apply is not called for
   it).  Everything else as vcg_conv_fwd_in (y, this conv's own statistics, `saved`).  The operand's magnitude is bounded by
   sqrt(H * W) instead of measured.  Exists where vcg_conv_pre_ok(cd) says 1 — the Winograd input transform (the D2..D4, R and U1
   layers at the training sizes); elsewhere it returns an error and the caller runs vcg_in_apply + vcg_conv_fwd_in.  The weight
   gradient of such a layer must come from `saved` (vcg_conv_wgrad_saved): there is no normalised x to re-read. */
int vcg_conv_pre_ok(const int32_t* cd);
int vcg_conv_fwd_in_pre(const float* t_prev, const float* pre_mean, const float* pre_rstd, int pre_act, const float* wf,
                        const float* bias, float* y, float* mean, float* rstd, float eps, float* saved, const int32_t* cd,
                        void* ws, size_t ws_bytes, void* stream);
/* dx = conv^T(dy) including the adjoint of the reflect padding.  Every element of dx is written: the pad channels
   dx[..., cin_log:] as exact zeros (tests/test_gpu_conv_plans.py checks it on every launch plan). */
size_t vcg_conv_dgrad_workspace(const int32_t* cd);
int vcg_conv_dgrad(const float* dy, const float* wf, float* dx, const int32_t* cd,
                   void* ws, size_t ws_bytes, void* stream);
int vcg_conv_dgrad_h(const float* dy, const float* wf, float* dx, const int32_t* cd,
                     void* ws, size_t ws_bytes, uint64_t dy_amax, void* stream);
/* gw_oihw += x^T dy (split-K slabs in ws, deterministic reduce); gbias += sum(dy).
   gbias may be NULL.                                                         */
size_t vcg_conv_wgrad_workspace(const int32_t* cd);
int vcg_conv_wgrad(const float* x, const float* dy, float* gw_oihw, float* gbias,
                   const int32_t* cd, void* ws, size_t ws_bytes, void* stream);
/* vcg_conv_wgrad with the forward state vcg_conv_fwd_in kept in `saved` (NULL: identical to vcg_conv_wgrad). */
int vcg_conv_wgrad_saved(const float* x, const float* dy, float* gw_oihw, float* gbias, const float* saved,
                         const int32_t* cd, void* ws, size_t ws_bytes, void* stream);
int vcg_conv_wgrad_saved_h(const float* x, const float* dy, float* gw_oihw, float* gbias, const float* saved,
                           const int32_t* cd, void* ws, size_t ws_bytes, uint64_t x_amax, uint64_t dy_amax, void* stream);

/* nn.InstanceNorm2d(eps=1e-5, affine=False) — Networks.py:61,88,102,105,123 -- */
size_t vcg_in_workspace(int N, int HW, int C);
int vcg_in_stats(const float* t, float* mean, float* rstd, int N, int HW, int C, float eps,
                 void* ws, size_t ws_bytes, void* stream);
/* out = post_act((t-mean)*rstd) [+ residual]; shuffle=1 stores through
   nn.PixelShuffle(2) (Networks.py:121): out is (N,2H,2W,C/4).                */
int vcg_in_apply(const float* t, const float* mean, const float* rstd, const float* residual,
                 float* out, int N, int H, int W, int C, int post_act, int shuffle, void* stream);
int vcg_in_apply_h(const float* t, const float* mean, const float* rstd, const float* residual,
                   float* out, int N, int H, int W, int C, int post_act, int shuffle, uint64_t* out_amax, void* stream);
/* dt = epi_act'(t) * IN-backward(post_act'(.) * g); g is in `out` layout.   */
int vcg_in_bwd(const float* g, const float* t, const float* mean, const float* rstd, float* dt,
               int N, int H, int W, int C, int epi_act, int post_act, int shuffle,
               void* ws, size_t ws_bytes, void* stream);
int vcg_in_bwd_h(const float* g, const float* t, const float* mean, const float* rstd, float* dt,
                 int N, int H, int W, int C, int epi_act, int post_act, int shuffle,
                 void* ws, size_t ws_bytes, uint64_t* dt_amax, void* stream);
/* vcg_in_bwd that also ACCUMULATES sum over (n, pixel) of dt into gbias[0 .. c_log): the bias gradient of the convolution in front
   of this InstanceNorm when an activation sits between the two (conv -> ReLU -> IN, Networks.py:93-95, 110-111, 128-130; with no
   activation between them it is identically zero) — from the pass that writes dt, instead of a pass of its own inside
   vcg_conv_wgrad (hand that call gbias = NULL).  dt_amax: as vcg_in_bwd_h (may be NULL).  Same workspace. */
int vcg_in_bwd_bias(const float* g, const float* t, const float* mean, const float* rstd, float* dt,
                    int N, int H, int W, int C, int epi_act, int post_act, int shuffle, float* gbias, int c_log,
                    void* ws, size_t ws_bytes, uint64_t* dt_amax, void* stream);
/* nn.PixelShuffle(2) — Networks.py:121 — as a copy: (N,H,W,C) -> (N,2H,2W,C/4); inverse=1 is its backward */
int vcg_pixel_shuffle(const float* src, float* dst, int N, int H, int W, int C, int inverse, void* stream);
/* dt = g * act'(t) where t is the activation OUTPUT (blocks without a norm). */
int vcg_act_bwd(const float* g, const float* t, float* dt, size_t n, int act, void* stream);
int vcg_act_bwd_h(const float* g, const float* t, float* dt, size_t n, int act, uint64_t* dt_amax, void* stream);

/* Helpers of the fused mu / logvar convolution (Networks.py:219-222: both convolutions read one map — they run as ONE
   convolution with 2 x latent output channels).  NHWC rows of ca + cb floats <-> rows of ca and rows of cb (multiples of 4;
   vcg_chan_cat: a NULL source reads as zeros); vcg_add_into: dst += src, src = 0 (n a multiple of 4, 16-byte aligned) — the
   fused kernel's weight gradient handed to the two parameters' own gradient buffers. */
int vcg_chan_split(const float* src, float* a, float* b, size_t rows, int ca, int cb, void* stream);
int vcg_chan_cat(const float* a, const float* b, float* dst, size_t rows, int ca, int cb, void* stream);
int vcg_add_into(float* dst, float* src, size_t n, void* stream);

/* VariationalEncoderBlock.forward — Networks.py:219-227 -------------------- */
/* lvc = clamp(lv,-10,10); z = mu + eps*exp(0.5*lvc). eps==NULL: eps is drawn
   on device (Philox4x32-10 + Box-Muller, (seed, offset)) and written to eps_out. */
int vcg_reparam_fwd(const float* mu, const float* lv, const float* eps, float* eps_out,
                    float* z, float* lvc, size_t n, uint64_t seed, uint64_t offset, void* stream);
/* dmu = gz ; dlv = (gz*eps*0.5*exp(0.5*lvc) + glvc) * [-10<=lv<=10]; glvc may be NULL */
int vcg_reparam_bwd(const float* gz, const float* glvc, const float* eps, const float* lv,
                    float* dmu, float* dlv, size_t n, void* stream);
int vcg_randn(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream);
int vcg_rand_uniform(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream);

/* Losses.py ---------------------------------------------------------------- */
size_t vcg_reduce_workspace(size_t n);
/* nn.L1Loss — Losses.py:21-24,34-39,53-65: out[0] = sum|a-b| / n_logical     */
int vcg_l1_fwd(const float* a, const float* b, float* out, size_t n_phys, size_t n_logical,
               void* ws, size_t ws_bytes, void* stream);
/* ga = sign(a-b) * gout[0] / n_logical ; gb (optional) = -ga                 */
int vcg_l1_bwd(const float* a, const float* b, const float* gout, float* ga, float* gb,
               size_t n_phys, size_t n_logical, void* stream);
/* nn.MSELoss vs a constant — Losses.py:78-83,97-102: out[0]=mean((d-c)^2), out[1]=mean(d) */
int vcg_mse_const_fwd(const float* d, float target, float* out, size_t n, void* stream);
int vcg_mse_const_bwd(const float* d, float target, const float* gout, float* gd, size_t n, void* stream);
/* The adversarial terms of one discriminator's real / fake logit pair under a selectable objective (new: the reference has the
   LSGAN of vcg_mse_const_* alone, which stays the default path).  real, fake: dense fp32 logits, n_real and n_fake of them; a side
   is present with a pointer and a count or absent with null and 0, not both absent.  smooth: the one-sided label smoothing s of
   the discriminator's real term, finite, 0 <= s < 0.5, and 0 with the hinge.  Each term is the mean over its tensor of, with
   sp(t) = max(t, 0) + log1p(exp(-|t|)):
     objective               D real                     D fake          G real   G fake
     VCG_GAN_LSGAN           (z - (1 - s))^2            z^2             z^2      (z - 1)^2
     VCG_GAN_HINGE           max(0, 1 - z)              max(0, 1 + z)   z        -z
     VCG_GAN_LOGISTIC        (1 - s) sp(-z) + s sp(z)   sp(z)           sp(z)    sp(-z)
     out[0..6) = g_real, g_fake, d_real, d_fake, mean(real), mean(fake); the slots of an absent side are written as 0
   One launch, workgroup 0 on `real` and workgroup 1 on `fake`: summands and sums in double, a fixed combination order, no
   atomics, one rounding to fp32 at the store.  A NaN logit gives NaN terms; an infinite one the limit.  csrc/gan_terms.hip. */
enum { VCG_GAN_LSGAN = 0, VCG_GAN_HINGE = 1, VCG_GAN_LOGISTIC = 2 };
int vcg_gan_terms_fwd(const float* real, size_t n_real, const float* fake, size_t n_fake, int objective, double smooth,
                      float* out, void* stream);
/* g_out: a host table of four device scalars, the upstream gradients of g_real, g_fake, d_real, d_fake; a null entry = that term
   is not differentiated (the generator and the discriminator phase of a step each set their own).  One elementwise launch:
     g_real[i] = (g_out[0] G'(real[i]) + g_out[2] D'(real[i])) / n_real;  g_fake[i] likewise from g_out[1], g_out[3], n_fake
   evaluated in double and rounded once; the hinge's derivative at its kink (z = 1 real, z = -1 fake) is 0.  A present side's
   buffer is written whole (zeros where both its entries are null); an absent side's may be null. */
int vcg_gan_terms_bwd(const float* real, size_t n_real, const float* fake, size_t n_fake, int objective, double smooth,
                      const float* const* g_out, float* g_real, float* g_fake, void* stream);
/* Discriminator feature-matching loss (new: the reference has no such term).  n_layers in 1..VCG_FM_MAX_LAYERS layers; layer l is
   fake[l], real[l]: rows[l] x cp fp32, the networks' NHWC buffers with rows = N h w, channels[l] logical channels at pitch
   cp = 4 ceil(channels / 4) (the channel the fastest index), 16-byte aligned, pad lanes zero in both.  With L = n_layers and
   k_l = 1 / (L rows_l channels_l):
     VCG_FM_PAIR   out[0] = sum_l k_l sum_e |fake_l[e] - real_l[e]|                 the mean over the layers of their L1 means
     VCG_FM_MEAN   out[0] = sum_l k_l rows_l sum_c |D_lc|,  D_lc = (1 / rows_l) sum_rows (fake_l - real_l)[row, c]
                   signs[0 .. sum_l cp_l) = sign(D_lc), layer after layer at the layer's pitch (0 in the pad lanes), 16-byte aligned,
                   kept by the caller for vcg_feature_match_bwd (null is accepted in the pair mode, which stores none)
   Summands and sums in double, combined in a fixed order by further launches, no atomics, one rounding to fp32 at the store: the
   same input gives the same bits.  A NaN anywhere in a layer gives a NaN result.  ws: vcg_feature_match_workspace(...) bytes (0
   and vcg_last_error for bad arguments), 16-byte aligned.  vcg_feature_match_chunk(mode, channels): the work one workgroup takes
   at a time — float4s of a layer per chunk (pair), rows per slab of a layer with that many channels (mean); what the tests place
   their sizes around.  Refused (nothing launched): n_layers outside 1..4, an empty layer, a null pointer.  csrc/feature_match.hip. */
enum { VCG_FM_PAIR = 0, VCG_FM_MEAN = 1, VCG_FM_MAX_LAYERS = 4 };
size_t vcg_feature_match_chunk(int mode, int channels);
size_t vcg_feature_match_workspace(const size_t* rows, const int* channels, int n_layers, int mode);
int vcg_feature_match_fwd(const float* const* fake, const float* const* real, const size_t* rows, const int* channels,
                          int n_layers, int mode, float* out, float* signs, void* ws, size_t ws_bytes, void* stream);
/* The real side is a constant of the term.  One launch over all layers: with c_l = (float)((double)g_out[0] k_l), g_fake[l] =
   c_l sign(fake_l - real_l) element by element (pair; fake and real are read again) or c_l sign(D_lc) broadcast over the rows
   (mean; `signs` of the forward, fake and real may be null), sign(0) = 0, pad lanes 0, written whole.  A null g_fake[l]: that layer
   needs no gradient and is skipped; all null: nothing is launched.  g_out is read on the device. */
int vcg_feature_match_bwd(const float* const* fake, const float* const* real, const float* signs, const float* g_out,
                          float* const* g_fake, const size_t* rows, const int* channels, int n_layers, int mode, void* stream);
/* KLDivergenceLoss — Losses.py:115-121                                       */
int vcg_kl_fwd(const float* mu, const float* lv, float* out, size_t n,
               void* ws, size_t ws_bytes, void* stream);
int vcg_kl_bwd(const float* mu, const float* lv, const float* gout, float* gmu, float* glv,
               size_t n, void* stream);
/* The same term (Losses.py:115-121) with a free-bits floor per latent channel (new: the reference has none; Kingma et al. 2016).
   mu, lv: rows x cp fp32, the networks' NHWC latent with rows = N h w, c logical channels at pitch cp (a multiple of 4, the
   channel the fastest index), 16-byte aligned.  Per element k = -0.5 (1 + l - mu^2 - exp(l)), l = clamp(lv, -10, 10);
   KL_ch = mean over the rows of k.  A channel's gate is closed iff klc[ch] <= floor (a tie is closed; a NaN leaves it open).
     out3[0] = (1 / c) sum_ch max(KL_ch, floor)      the floored objective
     out3[1] = (1 / c) sum_ch KL_ch                  vcg_kl_fwd's mean in another summation order
     out3[2] = the number of channels whose gate is open
     klc[0 .. c) = KL_ch, kept by the caller for vcg_kl_fb_bwd
   Pad lanes ch >= c are never summed, never counted in c, and get gradient 0.  floor: finite and >= 0.  ws:
   vcg_kl_fb_workspace(rows, cp) bytes (0 and vcg_last_error for bad arguments), 16-byte aligned: one partial per (row slab,
   channel), summed per channel in slab order in double by a final launch.  No atomics: the same input gives the same bits.
   csrc/kl_free_bits.hip. */
size_t vcg_kl_fb_workspace(size_t rows, int cp);
int vcg_kl_fb_fwd(const float* mu, const float* lv, float* out3, float* klc, size_t rows, int c, int cp, float floor,
                  void* ws, size_t ws_bytes, void* stream);
/* With s = gout[0] / (rows c) where the channel's gate is open (recomputed from klc and floor: no mask is stored), else 0:
   gmu = mu s;  glv = -0.5 (1 - exp(l)) s where lv lies inside [-10, 10], else 0 (vcg_kl_bwd's rule).  Both rows x cp, written
   whole, pad lanes 0; gout is read on the device. */
int vcg_kl_fb_bwd(const float* mu, const float* lv, const float* gout, const float* klc, float* gmu, float* glv,
                  size_t rows, int c, int cp, float floor, void* stream);
/* Structural loss (new: the reference trains on pixel-wise terms only): out[0] = 1 - mean SSIM(a, b) over the N images, the 3
   logical channels and the (H - 10)(W - 10) valid positions of an 11 x 11 Gaussian window (sigma 1.5, normalised to sum 1,
   C1 = 0.01^2, C2 = 0.03^2, population moments): vcg_image_metrics's definition without the clamp of either operand.  a
   (generated), b (target): (N, H, W, 4) fp32, the networks' layout, 16-byte aligned, channel 3 never read into a sum; H, W >= 11
   independent.  ws: vcg_ssim_loss_workspace(N, H, W) bytes = N ceil((H - 10) / 16) ceil((W - 10) / 16) doubles rounded up to 16
   bytes (0 and vcg_last_error for bad sizes), 16-byte aligned: each tile's partial sum goes to a slot of its own and a final
   pass sums the slots in a fixed order — no float atomics, the same input gives the same bits.  csrc/ssim_loss.hip. */
size_t vcg_ssim_loss_workspace(int N, int H, int W);
int vcg_ssim_loss_fwd(const float* a, const float* b, float* out, int N, int H, int W, void* ws, size_t ws_bytes,
                      void* stream);
/* ga = gout[0] * d loss / d a, (N, H, W, 4) with channel 3 = 0, written for every pixel; gout is read on the device.  With
   B = dS/dvar_a, C = dS/dcov_ab, A = dS/dmu_a - 2 mu_a B - mu_b C per position and M = 3 N (H - 10)(W - 10):
   ga(q) = -gout / M [ (w * A)(q) + 2 a(q) (w * B)(q) + b(q) (w * C)(q) ], * the transposed 11-tap filter over the valid
   positions.  The coefficients are recomputed from a and b (a 20-pixel halo per 16 x 16 pixel tile): no workspace.  There is
   no gradient with respect to b. */
int vcg_ssim_loss_bwd(const float* a, const float* b, const float* gout, float* ga, int N, int H, int W, void* stream);
/* Multi-scale structural loss (new: the reference has no such term): MS-SSIM (Wang, Simoncelli & Bovik 2003) over K = `scales`
   in 1..5 levels of a 2 x 2 mean pyramid, H_{j+1} = H_j / 2, W_{j+1} = W_j / 2 (a last odd row or column is dropped), level 0 the
   images; window, constants, layout and alignment of vcg_ssim_loss_fwd; min(H, W) >> (K - 1) >= 11 (the refusal names the largest
   K the size allows).  Per level, image n and channel c, over the level's valid positions:
     f_j = mean((2 s_ab + C2) / (s_a^2 + s_b^2 + C2)) for j < K - 1 (contrast-structure),   f_{K-1} = mean(S) (the full SSIM),
     MS(n, c) = prod_j max(f_j, 1e-4)^{w_j},  w = the first K of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) over their sum,
     out[0] = 1 - mean over (n, c) of MS.
   K = 1 is the structural loss wherever every per-channel mean is above 1e-4.  ws: vcg_msssim_loss_workspace(N, H, W, scales)
   bytes (0 and vcg_last_error for bad arguments), 16-byte aligned: the pooled levels of a and b, one gradient map per pooled
   level, the per-(n, c, tile) slots of every level, the factors f and the table coef[n][c][j] = d out / d f_j (0 where f_j was
   clamped: a clamped factor passes no gradient, as torch.clamp).  Slots summed in a fixed order, no float atomics: the same
   input gives the same bits.  csrc/msssim_loss.hip. */
size_t vcg_msssim_loss_workspace(int N, int H, int W, int scales);
/* new: the reference has no such term.  The forward defined above; it leaves in ws what vcg_msssim_loss_bwd reads. */
int vcg_msssim_loss_fwd(const float* a, const float* b, float* out, int N, int H, int W, int scales, void* ws, size_t ws_bytes,
                        void* stream);
/* new: the reference has no such term.  ga = gout[0] * d out / d a, (N, H, W, 4) with channel 3 = 0, written for every pixel;
   gout is read on the device.  ws: the workspace the forward of the SAME a, b, scales left (its pooled levels and coef are read,
   its gradient maps written).  Coarse to fine, one launch per level: vcg_ssim_loss_bwd's recomputation with the level's
   coefficients (of the contrast-structure part alone for j < K - 1) scaled by gout coef[n][c][j] / positions_j, plus the pooling
   adjoint: pixel (y, x) with y < 2 H_{j+1}, x < 2 W_{j+1} receives 1/4 of level j + 1's gradient at (y / 2, x / 2).  There is no
   gradient with respect to b. */
int vcg_msssim_loss_bwd(const float* a, const float* b, const float* gout, float* ga, int N, int H, int W, int scales, void* ws,
                        size_t ws_bytes, void* stream);
/* Gradient-matching loss (new: the reference has no edge term): an L1 on the horizontal and vertical finite differences of
   d = a - b at S = `scales` in 1..4 subsampled scales (Eigen & Fergus 2015; Li & Snavely 2018).  With d_s[i, j] = d[i 2^s, j 2^s],
   H_s = ceil(H / 2^s), W_s = ceil(W / 2^s), s = 0 .. S - 1, and the sums taken over the N images and the 3 logical channels:
     X_s = sum |d_s[i, j+1] - d_s[i, j]| over i < H_s, j < W_s - 1,   M_sx = 3 N H_s (W_s - 1)
     Y_s = sum |d_s[i+1, j] - d_s[i, j]| over i < H_s - 1, j < W_s,   M_sy = 3 N (H_s - 1) W_s
     out[0] = 1 / S  sum_s (X_s / M_sx + Y_s / M_sy);  a direction with no pair (M = 0) contributes 0, the divisor stays S.
   a (generated), b (target): (N, H, W, 4) fp32, the networks' layout, 16-byte aligned, channel 3 never read into a sum; H, W >= 1
   independent.  ws: vcg_grad_loss_workspace(N, H, W, scales) bytes = N ceil(H / 32) ceil(W / 32) 2 scales doubles rounded up to
   16 bytes (0 and vcg_last_error for bad sizes), 16-byte aligned: the 2 S partial sums of each 32 x 32 tile of pixels go to slots
   of the tile's own and a final pass sums them in a fixed order — no float atomics, the same input gives the same bits.
   csrc/grad_loss.hip. */
size_t vcg_grad_loss_workspace(int N, int H, int W, int scales);
int vcg_grad_loss_fwd(const float* a, const float* b, float* out, int N, int H, int W, int scales, void* ws, size_t ws_bytes,
                      void* stream);
/* ga = gout[0] * d loss / d a, (N, H, W, 4) with channel 3 = 0, written for every pixel; gout is read on the device.  The pixel
   (y, x) belongs, at every scale s with 2^s | y and 2^s | x, to the pairs with its neighbours 2^s to the left, right, above and
   below, where those lie inside the image:
   ga(y, x) = gout / S sum_s [ (sgn(left pair) - sgn(right pair)) / M_sx + (sgn(upper pair) - sgn(lower pair)) / M_sy ],
   a pair's sign that of (its right or lower pixel's d) - (its left or upper pixel's d), sgn(0) = 0.  No workspace.  There is no
   gradient with respect to b. */
int vcg_grad_loss_bwd(const float* a, const float* b, const float* gout, float* ga, int N, int H, int W, int scales,
                      void* stream);
/* Focal frequency loss (new: the reference has no spectral term; Jiang et al., ICCV 2021, at its defaults patch_factor 1 and no
   ave_spectrum / log_matrix / batch_matrix).  With d = a - b and, for each of the 3 N planes (image n, logical channel c),
     D = F_H d F_W,  F_n[j, k] = exp(-2 pi i j k / n) / sqrt(n)   (the orthonormal 2-D DFT),   p = |D|^2,
     m = |D|^alpha  (alpha = 0: m = 1, also where D = 0),
     w = m / max over the plane of m, 0 where that max is 0, clamped to [0, 1], a constant for the gradient:
     out[0] = 1 / (3 N H W)  sum over planes and frequencies of  w p.
   a (generated), b (target): (N, H, W, 4) fp32, the networks' layout, 16-byte aligned, channel 3 never read; H, W in
   1 .. VCG_FREQ_MAX_SIDE independent (no power of two asked for: the DFT is two matrix products on the fp32 MFMA, the twiddles
   looked up at (j k) mod n in a table of n entries built per call), N <= 21845; alpha finite and >= 0.  A NaN operand gives NaN.
   spec: vcg_freq_loss_spectrum(N, H, W) bytes, 16-byte aligned: the state the forward keeps for the backward (the spectrum and
   the plane maxima, layout private to the library).  ws: vcg_freq_loss_workspace(N, H, W) bytes of scratch, 16-byte aligned,
   one size for both directions.  Both sizes are multiples of 16; 0 and vcg_last_error for bad sizes.  Partial sums go to slots
   of their own and are added in a fixed order — no float atomics, the same input gives the same bits.  csrc/freq_loss.hip. */
#define VCG_FREQ_MAX_SIDE 2048
size_t vcg_freq_loss_workspace(int N, int H, int W);
size_t vcg_freq_loss_spectrum(int N, int H, int W);
int vcg_freq_loss_fwd(const float* a, const float* b, float* out, int N, int H, int W, float alpha, void* spec,
                      size_t spec_bytes, void* ws, size_t ws_bytes, void* stream);
/* ga = gout[0] * d loss / d a = gout[0] 2 / (3 N H W) Re(F_H^H (w . D) F_W^H), (N, H, W, 4) with channel 3 = 0, written for
   every pixel; gout is read on the device.  Reads spec as the forward with the same N, H, W, alpha left it, not a and b.
   There is no gradient with respect to b. */
int vcg_freq_loss_bwd(const void* spec, size_t spec_bytes, const float* gout, float* ga, int N, int H, int W, float alpha,
                      void* ws, size_t ws_bytes, void* stream);
/* out[0] = sum_i w[i]*(*s[i]) ; the composite loss lines Networks.py:941,2012-2018 */
int vcg_lincomb_fwd(const float* const* s, const float* w, int count, float* out, void* stream);

/* spectral_norm(nn.Conv2d(512,1,16)) — Networks.py:248 ---------------------- */
/* one power iteration exactly as torch.nn.utils.spectral_norm in train mode:
   v<-normalize(W^T u), u<-normalize(W v), sigma=u.(W v); wsn (NHWC-K order) = W/sigma.
   ws: >= 8 bytes of device scratch (two scalars handed from the reduction to the all-CU apply pass) */
int vcg_sn_prepare(const float* w_orig_oihw, float* u, float* v, float* sigma, float* wsn_k,
                   int C, int KH, int KW, int update_uv, void* ws, size_t ws_bytes, void* stream);
/* out[n] = <x[n,:], wsn_k> + bias[0]                                          */
int vcg_fullmap_fwd(const float* x, const float* wsn_k, const float* bias, float* out,
                    int N, size_t K, void* stream);
/* dx[n,:] = g[n]*wsn_k (dx may be NULL)                                       */
int vcg_fullmap_dgrad(const float* g, const float* wsn_k, float* dx, int N, size_t K, void* stream);
/* gw_orig_oihw += d(W/sigma)^T applied to (sum_n g[n] x[n,:]); gbias[0] += sum g */
int vcg_fullmap_wgrad(const float* g, const float* x, const float* wsn_k, const float* sigma,
                      const float* u, const float* v, float* gw_orig_oihw, float* gbias,
                      int N, int C, int KH, int KW, void* ws, size_t ws_bytes, void* stream);

/* The same layer on a map larger than its kernel — Networks.py:248 followed by .view(-1, 1).squeeze(1), Networks.py:269: a valid,
   stride-1 convolution with one output channel, the patch discriminator the reference becomes above 256 x 256.
   x (N, H, W, C) NHWC, wsn_k as vcg_sn_prepare writes it ((kh KW + kw) C + c), C % 4 == 0, KH <= H, KW <= W (kernels above
   16 rows or columns run as tiles of 16); OH = H - KH + 1, OW = W - KW + 1.  fp32 products and sums on the fp32 MFMA, no
   atomics, every sum in an order fixed by the shapes, and image n's results do not depend on the rest of the batch.
   ws: vcg_patch_head_workspace(...) bytes (one size for the three directions, a multiple of 16; 0 and vcg_last_error for bad
   dims or a map row too wide for the on-chip staging, some 400 pixels).  csrc/patch_head.hip. */
size_t vcg_patch_head_workspace(int N, int H, int W, int C, int KH, int KW);
/* out[(n OH + oy) OW + ox] = bias[0] + sum_{ky,kx,c} x[n, oy+ky, ox+kx, c] wsn_k[ky, kx, c] (bias may be NULL) — Networks.py:248, :269 */
int vcg_patch_head_fwd(const float* x, const float* wsn_k, const float* bias, float* out, int N, int H, int W, int C, int KH,
                       int KW, void* ws, size_t ws_bytes, void* stream);
/* dx[n, y, x, c] = sum_{oy,ox} g[n, oy, ox] wsn_k[y-oy, x-ox, c]: every element of dx written, none accumulated — the data
   gradient of Networks.py:248 */
int vcg_patch_head_dgrad(const float* g, const float* wsn_k, float* dx, int N, int H, int W, int C, int KH, int KW, void* stream);
/* gk[ky, kx, c] = sum_{n,oy,ox} g[n, oy, ox] x[n, oy+ky, ox+kx, c], then as vcg_fullmap_wgrad: gw_orig_oihw += d(W/sigma)^T gk,
   gbias[0] += sum of all N OH OW entries of g (gbias may be NULL) — the weight gradient of Networks.py:248 */
int vcg_patch_head_wgrad(const float* g, const float* x, const float* wsn_k, const float* sigma, const float* u, const float* v,
                         float* gw_orig_oihw, float* gbias, int N, int H, int W, int C, int KH, int KW, void* ws, size_t ws_bytes,
                         void* stream);

/* Input transforms on the device — the torchvision pipelines of train.py:184-190, 248-262, 309-319 ------------------------- */
/* RandomHorizontal/VerticalFlip -> RandomResizedCrop(S, BICUBIC) | Resize((S,S)) -> ToTensor for N decoded uint8 HWC images
   packed in `arena`.  params[n][16] (device, int32): source offset lo, hi; source H, W; crop box y0, x0, h, w in
   FLIPPED-image coordinates; flip_h; flip_v; filter (0 bicubic, 1 bilinear); source kind (0: uint8 RGB in `arena`, offset in
   bytes; 1: float4 pixels in [0, 1] in `fsrc` — what vcg_input_prejitter left — offset in pixels; fsrc may be NULL when no
   sample uses it).  Pillow's antialiased convolution resize in floating point.  out: (N, S, S, 4) fp32, channel 3 = 0 — the
   layout every network entry point takes.                                                                                     */
int vcg_input_resample(const unsigned char* arena, const float* fsrc, const int32_t* params, float* out, int N, int S,
                       void* stream);
/* torchvision ColorJitter (tensor-path formulas) in place on (N, S, S, 4).  jitter[n][8] (device, fp32): enabled, brightness,
   contrast, saturation, hue factors, order code o0 + 4 o1 + 16 o2 + 64 o3 (0 brightness, 1 contrast, 2 saturation, 3 hue). */
int vcg_input_color_jitter(float* img, const float* jitter, int N, int S, void* stream);
/* ColorJitter on WHOLE decoded frames, before any crop — hypersim's colour modality (Data_Manager.py:164-171 applies
   color_transform first, then the spatial transform): unpacks N uint8 frames into float4 pixels in `fbuf` and jitters them
   there.  frames[n][8] (device, int32): arena byte offset lo, hi; pixel count; fbuf pixel offset lo, hi.  var[n][4]: fbuf
   pixel offset lo, hi; pixel count.  jitter[n][8] as above.                                                                   */
int vcg_input_prejitter(const unsigned char* arena, const int32_t* frames, const float* jitter, const int32_t* var,
                        float* fbuf, int N, void* stream);

/* Evaluation (test.py) --------------------------------------------------------------------------------------------------- */
/* Per-image quality of N outputs against N targets, both (N, S, S, 4) fp32 (the networks' layout, channels 0..2 used), the output
   clamped to [0, 1], the target as given: result[n][4] = l1, mse, psnr (10 log10(1 / mse); +inf when mse == 0), ssim (11 x 11
   Gaussian window, sigma 1.5, valid positions only, C1 = 0.01^2, C2 = 0.03^2, population moments, mean over positions and
   channels).  New: the reference has no metric.  S >= 11.  ws: at least N * ceil(S / 16)^2 * 4 floats (16-byte aligned); each
   tile's partial sums go to a slot of their own and are summed in a fixed order: the result of an image does not depend on the
   batch it is in.  csrc/metrics.hip. */
int vcg_image_metrics(const float* out, const float* target, float* result, int N, int S, float* ws, size_t ws_bytes,
                      void* stream);
/* (N, S, S, 4) fp32 -> contiguous (N, S, S, 3): fp32 clamp(0, 1), or (as_uint8) uint8 floor(255 v + 0.5) clipped to 0..255 — the
   images test.py:317-343 builds on the host with clamp / permute / numpy (figures), and the PNGs of --save_images. */
int vcg_to_display(const float* x, void* out, int N, int S, int as_uint8, void* stream);

/* Whole images of any size (translate.py) --------------------------------------------------------------------------------- */
/* N decoded frames of one size, uint8 (N, H, W, C) with C = 1 (grey, replicated), 3 or 4 (alpha dropped) -> (N, Hp, Wp, 4) fp32 in
   the networks' layout, channel 3 = 0: Pillow's decoded array -> torchvision ToTensor -> numpy.pad(mode="reflect") -> the
   pitch-4 copy, which the caller would otherwise make on the host.  Value: (float)v / 255.0f, a correctly rounded DIVISION as
   ToTensor's, not v * (1.0f / 255) (which differs in the last bit for 126 byte values).  The frame sits at (top, left) of the
   buffer; the border around it is filled by reflection WITHOUT repeating the edge pixel (row top - k holds source row k), so
   each of the four borders must be narrower than the frame (top < H, Hp - H - top < H, likewise in x).  translate.py rounds
   Hp, Wp up to multiples of 16 and centres the frame (top = (Hp - H) / 2).  src 4-byte aligned, out 16-byte aligned.
   csrc/image_io.hip. */
int vcg_image_load(const unsigned char* src, float* out, int N, int H, int W, int C, int Hp, int Wp, int top, int left,
                   void* stream);
/* vcg_to_display for the window (top, left, H, W) of an (N, Hp, Wp, 4) buffer -> contiguous (N, H, W, 3): the crop that undoes
   vcg_image_load's padding and the display conversion in one pass, with vcg_to_display's rounding (for Hp = Wp = H = W and
   top = left = 0 the same bytes). */
int vcg_to_display_hw(const float* x, void* out, int N, int Hp, int Wp, int top, int left, int H, int W, int as_uint8,
                      void* stream);
/* vcg_image_metrics for the windows (top, left, H, W) of two (N, Hp, Wp, 4) buffers, H, W >= 11: the same definitions over the
   H x W window (SSIM's valid positions are the (H - 10)(W - 10) of the window; nothing outside it is read), the same kernel,
   the same tile slots summed in the same fixed order: for H = W = Hp = Wp = S it returns vcg_image_metrics's bits.
   ws: at least N * ceil(H / 16) * ceil(W / 16) * 4 floats.  csrc/metrics.hip. */
int vcg_image_metrics_hw(const float* out, const float* target, float* result, int N, int Hp, int Wp, int top, int left,
                         int H, int W, float* ws, size_t ws_bytes, void* stream);

/* torch.optim.Adam.step — call sites Networks.py:312,894,1928-1935 ---------- */
/* single-tensor torch formula on one flat buffer:
   m += (1-b1)(g-m); v = b2 v + (1-b2) g^2; p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)
   one_minus_beta1/2: 1 - beta computed in double by the caller and rounded once, as torch passes them to lerp_ / addcmul_
   g above is grad[i] * grad_scale (1 / world after a summing all-reduce).  Where that product is not exact in fp32 it enters m
   through one FMA and v through a double evaluation rounded once, so that v stays within 3 units of fp32 roundoff of the formula;
   for grad_scale 1 or a power of two the result is torch's fp32 sequence bit for bit. */
int vcg_adam_step(float* p, const float* g, float* m, float* v, size_t n,
                  float step_size, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2,
                  float eps, float bc2_sqrt, float grad_scale, void* stream);

/* Gradient clipping by global norm (new: the reference has none; torch.nn.utils.clip_grad_norm_'s definition) -------------- */
/* out (device, 16-byte aligned) receives four floats about the n gradients g (16-byte aligned):
   out[0] = |grad_scale| sqrt(sum g[i]^2), the 2-norm of the gradient vcg_adam_step would see (+inf where it exceeds fp32);
   out[1] = min(1, max_norm / (norm + 1e-6)), torch's formula and constant, evaluated in double from the unrounded norm and rounded
            once to fp32;
   out[2] = 1.0 if any g[i] is NaN or +-Inf, else 0.0 (decided from the elements, not from out[0]: a finite gradient whose norm
            saturates fp32 gives out[0] = +inf, out[2] = 0 and the correctly rounded tiny coefficient);
   out[3] = 0.
   Squares and sums are taken in double.  Workgroup b sums the floats [b GN_CHUNK, (b + 1) GN_CHUNK) of g, GN_CHUNK = 16384, into a
   slot of its own in ws; a second single-workgroup pass (256 lanes) sums the slots in a fixed order, adds the n % 4 last
   elements and writes out.  No float atomics; the grid depends on n alone: the same input gives the same bits on every call.
   max_norm finite and > 0, grad_scale finite.  n == 0 writes norm 0, coefficient 1, flag 0.
   ws: vcg_grad_norm_workspace(n) = max(1, ceil(floor(n / 4) / 4096)) * 8 bytes rounded up to a multiple of 16 (host arithmetic,
   no GPU needed), 16-byte aligned.  csrc/grad_clip.hip. */
size_t vcg_grad_norm_workspace(size_t n);
int vcg_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, float* out, void* ws, size_t ws_bytes,
                  void* stream);
/* vcg_adam_step with the clip decided on the device: clip = vcg_grad_norm's out.  clip[2] != 0: nothing is written (p, m, v keep
   their bits).  Otherwise vcg_adam_step with grad_scale replaced by fl32(grad_scale * clip[1]) (one fp32 multiply), the same
   arithmetic otherwise: for clip[1] == 1.0f vcg_adam_step's result bit for bit. */
int vcg_adam_step_clipped(float* p, const float* g, float* m, float* v, size_t n,
                          float step_size, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2,
                          float eps, float bc2_sqrt, float grad_scale, const float* clip, void* stream);

/* Averaged weights (new: the reference has none) — csrc/ema.hip -------------------------------------------------------------- */
/* One step of an exponential moving average e of the n parameters p, in place on e:
     e[i] = fmaf(w, p[i] - e[i], e[i]),   w = (float)(1 - decay), computed in double by the caller and rounded once.
   p is read only.  w == 1.0f copies (e[i] = p[i] exactly: the rounded p - e would not give p back); w == 0 launches nothing and
   leaves e bit for bit.  An element with e[i] == p[i] keeps its value for every w.
   skip: null, or the four floats vcg_grad_norm left on the device: where skip[2] != 0 (the gradient held a NaN / Inf, so
   vcg_adam_step_clipped wrote nothing) this call writes nothing either.
   One float4 per lane over grids of at most 2048 x 256 lanes, the n % 4 last elements one by one; vector loads and stores only,
   no atomics, no workspace: the same input gives the same bits on every call.
   Refused (non-zero, vcg_last_error, nothing launched): e or p null; e or p not 16-byte aligned; w NaN, infinite or outside
   [0, 1].  e and p must not overlap.  n == 0 is a no-op. */
int vcg_ema_update(float* e, const float* p, size_t n, float w, const float* skip, void* stream);
/* a[i] <-> b[i] for n 4-byte words in one pass (bit patterns move as they are: a NaN keeps its payload); twice is the identity.
   The launch shape of vcg_ema_update; 16 B of traffic per element.  Refused: a or b null, a or b not 16-byte aligned, ranges
   [a, a + n) and [b, b + n) that overlap.  n == 0 is a no-op. */
int vcg_swap(float* a, float* b, size_t n, void* stream);

/* Image history pool of the discriminators (new: replaces nothing in the reference, which trains its discriminators on the fakes
   of the current step only) — csrc/image_pool.hip -------------------------------------------------------------------------------
   The buffer of Shrivastava et al., "Learning from Simulated and Unsupervised Images through Adversarial Training" (CVPR 2017),
   as CycleGAN-style trainers use it: the discriminator is shown each new fake either as itself or exchanged against a stored one.
   fake, out: N images of elems contiguous floats each (any layout: the call is geometry-blind); pool: capacity slots of elems
   floats.  plan: N entries in HOST memory, read before the call returns and applied in order n = 0 .. N-1:
     -1                     keep:   out[n] = fake[n]
     s in [0, capacity)     swap:   out[n] = pool[s], then pool[s] = fake[n]
     -(2 + s)               store:  pool[s] = fake[n], out[n] = fake[n]; the slot's old content is not read (it may be uninitialised)
   Two entries may name one slot: the later one receives what the earlier one put there, and the slot ends up with the later fake.
   The plan travels in the kernel arguments, 64 entries per launch: nothing is uploaded or synchronised; N > 64 is several launches
   on `stream`.  A lane owns one element index and walks the samples in order, so a slot written and read again within a call is
   written and read by one lane.  Data moves as 32-bit words (a NaN keeps its payload); fake is read only; slots the plan does not
   name keep their bits.  Vector loads and stores only, no atomics, no workspace.
   Refused (non-zero, vcg_last_error, nothing launched): a null pointer; fake, pool or out not 16-byte aligned; N < 0;
   capacity < 1; elems == 0 with N > 0; a plan entry outside the three forms; any overlap between the ranges fake[N * elems],
   out[N * elems] and pool[capacity * elems].  N == 0 is a no-op. */
int vcg_pool_exchange(const float* fake, float* pool, float* out, const int32_t* plan, int N, size_t elems, int capacity,
                      void* stream);

/* The sampling translator (translate.py --samples K; new: the reference has no inference path) — csrc/sample_stats.hip -------- */
/* Broadcast reparameterisation for inference (new: the reference has no inference path): forward only.  mu, lv: N physical latent
   maps of `per` floats each (per a multiple of 4).  For the samples j = first .. first + k - 1 of the K of every map
     z[(n, j)] = mu[n] + temperature * eps[(n, j)] * exp(0.5 * clamp(lv[n], -10, 10)),
   z (and eps_out, if not NULL: the eps used) sample-major within a map for this chunk: (N, k, per).
   eps == NULL: drawn on the device; sample (n, j) uses the values vcg_randn writes for (seed, offset + (n K + j) per / 4), per
   values long — a draw depends on (seed, offset, n, j) only, never on how the K samples are split into chunks; the batch uses
   N K per / 4 counters.  eps != NULL: the chunk's (N, k, per) noise (parity runs).
   temperature == 1 and K == 1: z has the bits of vcg_reparam_fwd on the same eps; temperature == 0: z[(n, j)] = mu[n] exactly.
   16-byte loads and stores, grid-stride.  Refused (non-zero, vcg_last_error, nothing launched): mu, lv or z null; N, K or k < 1;
   first < 0 or first + k > K; per == 0 or per % 4 != 0; temperature NaN, infinite or negative; a pointer not 16-byte aligned. */
int vcg_reparam_many_fwd(const float* mu, const float* lv, const float* eps, float* eps_out, float* z, int N, int K, int first,
                         int k, size_t per, float temperature, uint64_t seed, uint64_t offset, void* stream);
/* Running statistics over samples (new: the reference has no inference path).  y: (N, k, pixels, 4) fp32, a decoder's output for
   one chunk of k samples per frame in the networks' layout; mean, m2: (N, pixels, 4) fp32, the running mean and the running sum of
   squared deviations of clamp(y, 0, 1) — the values the user sees.  Per element the samples j = 0 .. k - 1 are folded in that order
   with Welford's update, continuing from `seen` samples already folded:
     c = seen + j + 1;  d = x - mean;  mean += d / c;  m2 = fmaf(d, x - mean, m2)
   seen == 0 initialises the statistics: mean and m2 are not read and need not be cleared.  One loop body and no compiler-chosen
   contraction: an element's operation sequence is the same for every chunking, so K samples folded in one call or in several give
   the same bits.  Channel 3 of y is not read and is written as 0.  One element is one lane's float4: no reduction, no atomics.
   Refused: a null pointer; N or k < 1; seen < 0 or seen + k > 2^24; pixels == 0; a pointer not 16-byte aligned; mean == m2. */
int vcg_sample_accumulate(const float* y, float* mean, float* m2, int N, int k, int seen, size_t pixels, void* stream);
/* The spread map of `count` >= 2 folded samples (new: the reference has no inference path): per pixel of the window
   (top, left, H, W) of m2, an (N, Hp, Wp, 4) buffer vcg_sample_accumulate filled,
     s = sqrt((m2_0 + m2_1 + m2_2) / (3 (count - 1))),
   the RMS over the three channels of the unbiased sample standard deviation, evaluated in double.  out_f32: (N, H, W) fp32, s
   rounded once; out_u8: (N, H, W) uint8, floor(255 min(1, gain s) + 0.5); either may be NULL.  result[n]: the mean of s over image
   n's window, fp32, accumulated in double: each 16 x 16 tile writes its partial to a slot of its own in ws and a final pass sums an
   image's slots in a fixed order (csrc/metrics.hip's scheme) — no float atomics, and an image's result does not depend on the
   batch it is in.  Nothing outside the window is read.
   ws: vcg_spread_workspace(N, H, W) = N ceil(H / 16) ceil(W / 16) doubles rounded up to 16 bytes (0 and vcg_last_error for bad
   sizes; host arithmetic), 16-byte aligned.
   Refused: m2, result or ws null; count < 2; gain NaN, infinite or negative; N, H or W < 1; a window that leaves the buffer; m2 or
   ws not 16-byte aligned, out_f32 or result not 4-byte aligned; a workspace that is too small. */
size_t vcg_spread_workspace(int N, int H, int W);
int vcg_spread_display_hw(const float* m2, int count, float gain, float* out_f32, unsigned char* out_u8, float* result, int N,
                          int Hp, int Wp, int top, int left, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* The interpolating translator (translate.py --interpolate N; new: the reference has no inference path) — csrc/latent_path.hip.
   Latent maps are in the networks' physical layout, (h, w, pitch) fp32 with C <= pitch logical channels per pixel: `per` =
   h w pitch floats per map.  A pair p is (a[p], b[p]); a and b each point at P consecutive maps and are only read, so they may
   overlap: a = mu, b = mu + per makes the consecutive frames of one encoder batch the pairs, without a copy.  Pad lanes
   (channels C .. pitch - 1) never enter a sum or an output: a NaN there does no harm. */
#define VCG_LATENT_SLERP 0
#define VCG_LATENT_LERP 1
/* Below this sin(omega) the slerp uses the lerp coefficients.  sin(omega) < 1e-4 means the pair is within 1e-4 rad of parallel or
   antiparallel; for the parallel case sin((1 - t) omega) / sin(omega) = (1 - t) (1 + O(omega^2)), so the two coefficient sets
   differ by about omega^2 = 1e-8 relative, under the 6e-8 of fp32 rounding — the switch cannot be seen in z — while the division
   by sin(omega) stays far from 0 / 0.  Antiparallel maps have no unique great circle; the straight line is the fallback there too. */
#define VCG_SLERP_MIN_SIN 1e-4
/* out[p] = [sum a[p]^2, sum b[p]^2, sum a[p] b[p]] over the logical channels, (P, 3) doubles; every summand (exact: a product of
   two fp32 values) and every sum in double, because omega = acos(sum ab / sqrt(sum a^2 sum b^2)) loses half the digits of its
   argument near parallel pairs.  Wave shuffles, then LDS in wavefront order; each workgroup writes one partial to a slot of its
   own in ws and a final launch sums a pair's slots in a fixed order (csrc/metrics.hip's scheme): no atomics, the same bits on
   every call, and a pair's numbers do not depend on P or on the other pairs (the slot count is a function of per alone).
   ws: vcg_latent_stats_workspace(P, per) bytes (host arithmetic; 0 and vcg_last_error for P < 1, per == 0, per % 4 != 0 or
   per > 2^31).
   Refused (non-zero, vcg_last_error, nothing launched): a null pointer; P < 1; per == 0 or > 2^31; pitch % 4 != 0, C < 1,
   C > pitch or per % pitch != 0; a or b not 16-byte aligned, out or ws not 8-byte aligned; a workspace that is too small. */
size_t vcg_latent_stats_workspace(int P, size_t per);
int vcg_latent_pair_stats(const float* a, const float* b, double* out, int P, size_t per, int C, int pitch, void* ws,
                          size_t ws_bytes, void* stream);
/* The fractions j = first .. first + k - 1 of the T >= 2 uniform fractions t_j = j / (T - 1) of every pair's path:
     z[(p, j)] = ca a[p] + cb b[p],  z (P, k, per), fraction-major within a pair (the decoder-batch order of vcg_reparam_many_fwd).
   (ca, cb) of a (pair, j) are evaluated in double and rounded once to fp32:
     VCG_LATENT_LERP    (1 - t, t);
     VCG_LATENT_SLERP   omega = acos(clamp(sum ab / sqrt(sum a^2 sum b^2), -1, 1)) from `stats` (vcg_latent_pair_stats's (P, 3)),
                        ca = sin((1 - t) omega) / sin(omega), cb = sin(t omega) / sin(omega): the endpoints are not normalised, the
                        usual latent slerp; the lerp coefficients where sum a^2 == 0, sum b^2 == 0, sin(omega) < VCG_SLERP_MIN_SIN
                        or a stat is not finite.
   j == 0 writes a[p] and j == T - 1 writes b[p], bit for bit (a NaN keeps its payload, -0 its sign).  Elsewhere, in fp32,
     z = fmaf(ca, a, __fmul_rn(cb, b)):
   an explicit fused multiply-add over an explicit product, two roundings, no compiler-chosen contraction.  A value depends on
   (pair, j, T, mode) only, never on first or k: a path computed in one call or in chunks has the same bits.  Pad lanes of z are 0.
   coef_out, if not NULL: (P, k, 2) fp32, the (ca, cb) used ((1, 0) and (0, 1) at the two ends).  stats is not read by the lerp and
   may then be NULL.  z must not overlap a or b.
   16-byte loads and stores; a lane loads its float4 of a and of b once and keeps them in registers over the k fractions, whose
   coefficients the workgroup staged in LDS: (2 + k) per floats of traffic per pair.  Grid (blocks over per, pairs), grid-stride.
   Refused (non-zero, vcg_last_error, nothing launched): an unknown mode; a, b or z null, stats null with the slerp; P < 1;
   per == 0 or > 2^31; pitch % 4 != 0, C < 1, C > pitch or per % pitch != 0; T < 2; k < 1, first < 0 or first + k > T; a, b or z
   not 16-byte aligned, stats or coef_out not 8-byte aligned. */
int vcg_latent_path(const float* a, const float* b, const double* stats, float* z, float* coef_out, int P, int T, int first, int k,
                    size_t per, int C, int pitch, int mode, void* stream);

/* Sliced Wasserstein distance on Laplacian-pyramid patches (new: the reference compares unpaired runs by eye only; Karras et
   al., ICLR 2018, section 5) — csrc/swd.hip.  Forward only.  No float atomics: every call gives the same bits for the same input.
   The stages of one pyramid level, in order: vcg_swd_pyramid_level, vcg_swd_gather, vcg_swd_normalize, vcg_swd_project,
   vcg_sort_columns, vcg_swd_distance.  At most VCG_SWD_MAX_DESC descriptors per set and level: a sorted column lives in LDS. */
#define VCG_SWD_MAX_DESC 16384
/* One pyramid level from g, N images (N, S, S, 4) fp32 (channels 0..2 used; `clamp` != 0: clamped to [0, 1] first, level 0).
   With gk = [1, 4, 6, 4, 1] / 16, K = gk (x) gk and borders mirrored without repeating the edge (-k -> k, S-1+k -> S-1-k):
     g_next[i, j] = (K * g)[2i, 2j]                          (N, S/2, S/2, 4)
     lap = g - (4 K) * Z,  Z[2i, 2j] = g_next[i, j], 0 elsewhere   (N, S, S, 4)
   g_next == NULL: no coarser level; lap = g (clamped if asked).  Channel 3 of both outputs is 0.  S >= 8, even unless g_next is
   NULL; map sizes that are no multiple of the 32-pixel tile are exact at the borders.  The three buffers are distinct. */
int vcg_swd_pyramid_level(const float* g, float* g_next, float* lap, int N, int S, int clamp, void* stream);
/* Rows row_offset .. row_offset + count - 1 of out, a (rows, 147) fp32 matrix: the 7 x 7 x 3 patches of `level` ((N, S, S, 4))
   named by plan, `count` entries (image, top, left) in HOST memory, read before the call returns; a patch is flattened as
   (c, dy, dx).  The plan travels in the kernel arguments, 256 entries per launch.  Refused (nothing launched): an entry with
   image outside [0, N) or top / left outside [0, S - 7]; rows that leave the matrix.  count == 0 is a no-op. */
int vcg_swd_gather(const float* level, int N, int S, const int32_t* plan, int count, float* out, size_t row_offset,
                   size_t rows, void* stream);
/* out = (desc - mean_c) / std_c for the n x 147 descriptor matrix: per channel c (columns 49 c .. 49 c + 48), the mean and the
   population standard deviation over all n rows and the channel's 49 columns, taken in two passes in double (block slots summed
   in a fixed order); each element is evaluated in double and rounded once.  A constant channel has std exactly 0: its columns
   come out NaN.  out may be desc.  ws: vcg_swd_normalize_workspace(n) bytes (0 and vcg_last_error for n outside
   1 .. VCG_SWD_MAX_DESC), 16-byte aligned. */
size_t vcg_swd_normalize_workspace(int n);
int vcg_swd_normalize(const float* desc, float* out, int n, void* ws, size_t ws_bytes, void* stream);
/* out[j][r] = sum_k dirs[k][j] desc[r][k]: the (ndir, n) TRANSPOSE of desc (n, K) x dirs (K, ndir), so that one direction's
   projections are contiguous for the sort.  fp32 products and fp32 accumulation (v_mfma_f32_32x32x2_f32). */
int vcg_swd_project(const float* desc, const float* dirs, float* out, int n, int K, int ndir, void* stream);
/* Every column of an n x cols fp32 matrix sorted ascending over the rows; element (r, c) is at r * row_stride + c * col_stride
   in x and in out (dense: row_stride == 1 or col_stride == 1; out may be x).  One workgroup per column: a bitonic network in
   LDS over the keys padded with +inf to a power of two.  -0 and +0 compare equal; +-inf sort as values.  The network's shape
   depends on n alone: a column holding a NaN completes, unsorted, and the other columns are not affected.
   Refused (nothing launched): n outside 1 .. VCG_SWD_MAX_DESC. */
int vcg_sort_columns(const float* x, float* out, int n, int cols, size_t row_stride, size_t col_stride, void* stream);
/* out[0] = mean |a[i] - b[i]| over n floats, summed in double: block slots, then a fixed-order final sum.
   ws: vcg_swd_distance_workspace(n) bytes, 16-byte aligned. */
size_t vcg_swd_distance_workspace(size_t n);
int vcg_swd_distance(const float* a, const float* b, float* out, size_t n, void* ws, size_t ws_bytes, void* stream);

/* Sliced Wasserstein distance as a training loss between two image sets (new: a patch-distribution term that needs no pairing,
   no discriminator and no pretrained network) — csrc/swd_loss.hip; DESIGN.md, "Sliced Wasserstein training loss".  No float
   atomics: every call gives the same bits for the same input.  The stages of one level, forward: [vcg_swd_pool,]
   vcg_swd_grid_gather, vcg_swd_project, vcg_sort_columns_indexed (the generated set) / vcg_sort_columns (the target set),
   vcg_swd_pair_loss; backward: vcg_swd_project with the roles swapped, vcg_swd_grid_scatter, vcg_swd_pool_adjoint_add.
   Images are (N, H, W, 4) fp32 with channels 0..2 used.  At most VCG_SWD_LOSS_MAX_DESC descriptors per set and level: a column's
   keys and source rows are sorted together in 64 KiB of LDS. */
#define VCG_SWD_LOSS_MAX_DESC 8192
#define VCG_SWD_LOSS_MAX_LEVELS 3
/* The number of levels, at most VCG_SWD_LOSS_MAX_LEVELS, an H x W image has: level k + 1 exists while both sides of level k are
   even and their halves at least 16.  0 and vcg_last_error: a side under 16 or over 32768.  Host arithmetic. */
int vcg_swd_loss_levels(int H, int W);
/* The side s of the square cells an (N, H, W) level is cut into: the smallest s >= 8 with N floor(H / s) floor(W / s) <=
   VCG_SWD_LOSS_MAX_DESC.  0 and vcg_last_error: N < 1, a side under 16 or over 32768, or no s <= min(H, W) meets the cap.
   Host arithmetic. */
int vcg_swd_cell_side(int N, int H, int W);
/* out (N, H/2, W/2, 4) = the 2 x 2 mean of x (N, H, W, 4): the four values added in double, rounded once; channel 3 is 0.
   vcg_swd_pool_adjoint_add: fine (N, H, W, 4) += coarse (N, H/2, W/2, 4) / 4 at [y/2, x/2], channel 3 left alone.
   Refused (nothing launched): a null pointer; N outside 1..65535; an odd side, a half under 16, a side over 32768; buffers that
   are not 16-byte aligned or not distinct. */
int vcg_swd_pool(const float* x, float* out, int N, int H, int W, void* stream);
int vcg_swd_pool_adjoint_add(const float* coarse, float* fine, int N, int H, int W, void* stream);
/* The level (N, H, W, 4) is cut into cy x cx = floor(H / s) x floor(W / s) cells of s x s per image; cell (image, i, j) gives row
   (image cy + i) cx + j of out, an (N cy cx, 147) matrix: the 7 x 7 x 3 patch whose top left pixel is (i s + oy, j s + ox),
   flattened as (c, dy, dx).  Rows and columns past cy s, cx s belong to no cell.  The geometry travels by value: no host
   memory is read.
   vcg_swd_grid_scatter is the adjoint in gather form: out (N, H, W, 4) [pixel of patch element e of row r][c] =
   gdesc[r][e] * scale * (gscale ? gscale[0] : 1), gscale a device scalar; every other pixel and channel 3 are +0: it clears
   the map as it writes it.
   Refused (nothing launched): a null level / gdesc / out; N outside 1..65535; a side under 16 or over 32768; s under 8 or over
   min(H, W); oy or ox outside [0, s - 7]; N cy cx outside 1 .. VCG_SWD_LOSS_MAX_DESC; a scale that is not finite; out of the
   scatter not 16-byte aligned. */
int vcg_swd_grid_gather(const float* level, float* out, int N, int H, int W, int s, int oy, int ox, void* stream);
int vcg_swd_grid_scatter(const float* gdesc, const float* gscale, float scale, float* out, int N, int H, int W, int s, int oy,
                         int ox, void* stream);
/* vcg_sort_columns that remembers where each key came from: keys and rows (int32) have x's layout; column c of keys is column c
   of x ascending, rows[i] the row of x that keys[i] came from.  Pairs are ordered by (key, row): the result is that of a stable
   argsort.  One workgroup per column, a bitonic network in LDS over the pairs padded with (+inf, n ..) to a power of two; its
   shape depends on n alone.  A column holding a NaN completes and comes out as it came, rows = 0 .. n - 1: the rows of a
   column are a permutation of 0 .. n - 1 in every case, and the other columns are not affected.  keys may be x.
   Refused (nothing launched): a null pointer; n outside 1 .. VCG_SWD_LOSS_MAX_DESC; cols < 1; strides that are not those of a
   dense matrix; keys == rows. */
int vcg_sort_columns_indexed(const float* x, float* keys, int32_t* rows, int n, int cols, size_t row_stride, size_t col_stride,
                             void* stream);
/* One pass over a_sorted, b_sorted and perm_a, all (ndir, n) with a direction's n values contiguous:
     level = mean_{d,i} |a_sorted[d][i] - b_sorted[d][i]|, summed in double in block slots, then in a fixed order;
     total[0] = (accumulate ? total[0] : 0) + weight * level (a double on the device), out[0] = (float)total[0];
     gproj[d][perm_a[d][i]] = sign(a_sorted[d][i] - b_sorted[d][i]), sign(0) = 0, not scaled (an entry of perm_a outside
     [0, n) is skipped).
   ws: vcg_swd_pair_loss_workspace(n, ndir) bytes (0 and vcg_last_error on refused arguments), 16-byte aligned.
   Refused (nothing launched): a null pointer; n outside 1 .. VCG_SWD_LOSS_MAX_DESC; ndir outside 1..1024; a weight that is not
   finite; gproj aliasing an input; a workspace that is too small or misaligned. */
size_t vcg_swd_pair_loss_workspace(int n, int ndir);
int vcg_swd_pair_loss(const float* a_sorted, const float* b_sorted, const int32_t* perm_a, float* gproj, int n, int ndir,
                      double weight, int accumulate, double* total, float* out, void* ws, size_t ws_bytes, void* stream);
/* out = x, a (K, D) row-major matrix, with every column scaled to unit 2-norm: the sum of squares in double, each element
   evaluated in double and rounded once (a zero column comes out NaN).  One workgroup per column.  out may be x.
   Refused (nothing launched): a null pointer; K outside 1..65536; D outside 1..65535. */
int vcg_swd_unit_columns(const float* x, float* out, int K, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VCG_H */
