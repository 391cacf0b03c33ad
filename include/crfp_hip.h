/* libcrfp_hip.so -- C ABI of the MI355X-native (gfx950) CRFP recurrent x8 foveated-VSR path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  Every pointer is a
 * DEVICE pointer owned by the caller (e.g. PyTorch's caching allocator) unless the argument is
 * documented as host memory; the library never allocates, frees or retains device memory --
 * scratch arrives through `workspace` (size from the matching *_workspace_bytes query).  Kernels
 * are enqueued asynchronously on `stream` (a hipStream_t passed as void*); no entry point
 * synchronises the device.
 *
 * State kept between calls (all of it): per (host thread, device) ONE non-blocking HIP stream and a
 * small pool of timing-disabled events, created lazily by the first crfp_dsv_forward_clip /
 * crfp_dsv_stream_frame on that device.  The engine forks the state-independent part of each frame
 * onto that stream and joins it back with events before returning control of `stream`'s order, on
 * success AND on every error path, so for the caller each call behaves as if it ran on `stream`
 * alone (buffers may be reused once `stream` has drained).  Clips issued by one host thread on
 * several caller streams share that one side stream (their side work serialises; results are
 * unaffected).  CRFP_SIDE_STREAM=0 in the environment (read once) selects a single-stream
 * schedule that creates nothing.  A host thread that exits hands its table (stream + events) to the next
 * new thread -- without calling HIP -- so short-lived worker threads do not accumulate streams.
 * crfp_shutdown() destroys EVERY thread's side streams and events (call it when no library call is in
 * flight on any thread and the streams have drained); the next call re-creates them lazily.  Return value: 0 = success, negative = CRFP_E_* argument error,
 * positive = hipError_t of a failed launch.  crfp_last_error_string() describes the last failure
 * on the calling thread.  No exceptions cross the boundary.
 *
 * Reference interfaces replaced (paths relative to the reference repo eugenelet/CRFP):
 *   crfp_flow_warp_f32        model/CRFP.py:90-130   flow_warp()  (ATen grid_sampler_2d underneath)
 *   crfp_flow_warp_backward_f32  autograd of flow_warp (ATen grid_sampler_2d_backward and the normalisation in front of it)
 *   crfp_dcnv2_shared_backward_f32  autograd of DCN_module's repeat path (model/CRFP.py:341-350) without the tiled tensors
 *   crfp_dcnv2_forward_f32    model/CRFP.py:6,318-320,350  third-party dcn_v2.DCNv2.forward
 *   crfp_dcnv2_backward_f32   the same extension's backward (autograd of self.dcn(pre_x, offset, mask), model/CRFP.py:350)
 *   crfp_conv3x3_f32          every nn.Conv2d(k=3,s=1,p=1) on the path (e.g. model/CRFP.py:48-50,303-317)
 *   crfp_conv3x3_ex_backward_f32  autograd of those convs with their activation, cat and pixel (un)shuffle (ATen convolution_backward)
 *   crfp_upsample_bilinear_backward_f32 / crfp_avgpool2_backward_f32  autograd of those resizes and of nn.AvgPool2d(2, 2)
 *   crfp_charbonnier_f32 / _backward_f32  loss/loss.py:26-68,115-124 (masked Charbonnier loss and its autograd)
 *   crfp_upsample_bilinear_f32  nn.Upsample / F.interpolate(align_corners=False) (model/CRFP.py:808-812,1471-1478)
 *   crfp_fnet_*               model/CRFP.py:743-814  FNet.forward, :1483-1508 compute_flow
 *   crfp_dsv_*                model/CRFP.py:1387-1706 CRFP_DSV (ctor weights, forward) and the
 *                             one-frame-per-call variant model/CRFP_test.py:2114-2478
 *   crfp_simple_* / crfp_dense_*  model/CRFP.py:816-1099 CRFP_simple / :1101-1385 CRFP (clip forward) and their
 *                             one-frame-per-call variants model/CRFP_test.py:1184-1486 MRCF_simple_v13 / :1805-2113 v15
 *   crfp_psnr_partial_f32     utils.py:166-185,242-254,328-330 (psnr_cuda / bgr2ycbcr(y_only))
 *   crfp_window_scores_f32    test_video.py:23-63 foveated_metric (per-window PSNR / SSIM maps)
 *   crfp_frame_metrics_f32    trainer.py:348-369 / test_video.py:360-370 (per-frame, per-region PSNR / SSIM / PSNR-Y / SSIM-Y)
 *   crfp_gaze_prep_f32        test_video.py:335-358,371-375 (fv / mk / mk_fv / mk_out / mk_past / fg of one streamed frame)
 *   crfp_frame_ingest_u8      dataset/reds.py:196-203,306,409 (8-bit LR frame, fovea crop and rectangle -> lr / fv / mk)
 *   crfp_frame_export_u8      test_video.py:100-127,396-410 (y_only chroma merge, clip, round, uint8, HWC, RGB -> BGR)
 *   crfp_spynet_forward       model/CRFP.py:554-741 SPyNet.forward (+ SPyNetBasicModule, `conv` :145-152)
 *   crfp_convkxk_f32          model/CRFP.py:145-152 `conv`: ReLU -> nn.Conv2d(k, stride 1, pad k/2)
 *   crfp_upsample_bilinear_ac_f32  F.interpolate(..., bilinear, align_corners=True) (model/CRFP.py:647-651)
 */
#ifndef CRFP_HIP_H
#define CRFP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRFP_VERSION 201 /* major*10000 + minor*100 + patch */

/* error codes (negative) */
#define CRFP_E_BADARG (-1)      /* null pointer / non-positive size / unsupported combination */
#define CRFP_E_WORKSPACE (-2)   /* workspace missing or too small */
#define CRFP_E_UNSUPPORTED (-3) /* shape or mode outside what the kernels implement */
#define CRFP_E_STATE (-4)       /* engine used before weights were packed */

/* activations for crfp_conv3x3_f32: out = post_scale * act(conv + bias) */
#define CRFP_ACT_NONE 0
#define CRFP_ACT_RELU 1
#define CRFP_ACT_LRELU01 2 /* LeakyReLU(0.1) */
#define CRFP_ACT_TANH 3
#define CRFP_ACT_SIGMOID 4

#define CRFP_PAD_ZEROS 0
#define CRFP_PAD_BORDER 1

int crfp_version(void);
const char* crfp_last_error_string(void);
/* destroy every host thread's side streams / events (see "State kept between calls"); always 0 */
int crfp_shutdown(void);

/* ---- flow_warp: x[n,c,h,w] (NCHW f32), flow[n,h,w,2] = (dx,dy) pixels, out[n,c,h,w].
 * Bilinear backward warp, align_corners=True semantics of the reference (sample position =
 * pixel index + flow, routed through the [-1,1] normalisation in the same float32 order). */
size_t crfp_flow_warp_workspace_bytes(int n, int c, int h, int w);
int crfp_flow_warp_f32(const float* x, const float* flow, float* out, int n, int c, int h, int w,
                       int padding_mode, void* workspace, size_t workspace_bytes, void* stream);

/* ---- DCNv2 forward (stride 1): x[n,cin,h,w], offset[n,2*dg*k*k,h,w] ((dy,dx) interleaved per
 * tap per group), mask[n,dg*k*k,h,w], weight[cout,cin,k,k], bias[cout] -> out[n,cout,h,w].
 * k=3, pad=1, dil=1 only (every call site of the reference).  Fast paths: (cin=cout=32, dg=8)
 * on MFMA and (cin=cout=4, dg=1); other channel counts run a generic HIP kernel. */
size_t crfp_dcnv2_workspace_bytes(int n, int cin, int cout, int h, int w, int k, int dg);
int crfp_dcnv2_forward_f32(const float* x, const float* offset, const float* mask, const float* weight,
                           const float* bias, float* out, int n, int cin, int cout, int h, int w, int k,
                           int pad, int dil, int dg, void* workspace, size_t workspace_bytes, void* stream);

/* ---- DCNv2 backward: the gradients of crfp_dcnv2_forward_f32's out = bias + sum weight * mask * bilinear(x at offset) for a given
 * grad_out[n,cout,h,w]: grad_x[n,cin,h,w], grad_offset[n,2*dg*9,h,w], grad_mask[n,dg*9,h,w], grad_weight[cout,cin,3,3], grad_bias[cout]
 * (the bias itself is not an input: its gradient is the sum of grad_out).  The forward's semantics exactly: (dy, dx) interleaved per
 * (group, tap), a sample counts only when -1 < py < h and -1 < px < w, each corner zero-padded on its own, the sample multiplied by the
 * mask.  grad_offset is the derivative inside the bilinear cell the forward's floor picked (the right-hand derivative at integer
 * positions); corners and samples the forward drops contribute exactly 0, and a NaN or infinite offset counts as outside.  Offsets are
 * unbounded: every corner is checked before its 64-bit index is formed.
 * Outputs: a NULL output pointer means "not wanted" and its work is skipped (no clear and no scatter for a NULL grad_x, no reduction
 * pass when grad_weight and grad_bias are both NULL); all five NULL is CRFP_E_BADARG.  Every element of a wanted output is defined by
 * the call: the caller initialises nothing (grad_x is cleared on `stream` by the call), and the workspace needs no initialisation.
 * Domain: the forward's -- k = 3, pad = 1, dil = 1, cin % dg == 0 -- with cin, cout <= 64, (32, 32, dg 8) and (4, 4, dg 1) included;
 * anything else (also n > 65535, h > 262140) is CRFP_E_UNSUPPORTED and the size query returns 0.  A null input or a size < 1 is
 * CRFP_E_BADARG, a missing or short workspace CRFP_E_WORKSPACE; every argument error is returned before any HIP call.  Asynchronous
 * on `stream`, no host synchronisation.
 * Numbers: fp32 throughout (no split-fp16: gradients have no bounded range).  Determinism: grad_offset, grad_mask, grad_weight and
 * grad_bias are bitwise reproducible from run to run (plain stores; grad_weight / grad_bias through per-workgroup partial slabs in the
 * workspace added in a fixed order).  grad_x is NOT: it is a data-dependent scatter of float atomic adds, whose sum depends on the
 * order in which the adds arrive, so its last bits can differ between runs. */
size_t crfp_dcnv2_backward_workspace_bytes(int n, int cin, int cout, int h, int w, int k, int dg);
int crfp_dcnv2_backward_f32(const float* x, const float* offset, const float* mask, const float* weight, const float* grad_out,
                            float* grad_x, float* grad_offset, float* grad_mask, float* grad_weight, float* grad_bias,
                            int n, int cin, int cout, int h, int w, int k, int pad, int dil, int dg,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- DCNv2 with ONE (dy, dx) and ONE mask per pixel shared by the 9 taps (cin = cout = 4, deformable_groups = 1): what
 * DCN_module(repeat=True) computes after tiling its 2 + 1 channels 9x (model/CRFP.py:341-347,350); the tiled tensors never exist.
 * offset [n,2,h,w] = (dy, dx), mask [n,1,h,w]. */
size_t crfp_dcnv2_shared_workspace_bytes(int n, int c, int h, int w);
int crfp_dcnv2_shared_f32(const float* x, const float* offset, const float* mask, const float* weight, const float* bias, float* out,
                          int n, int cin, int cout, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

/* ---- backward of crfp_dcnv2_shared_f32: crfp_dcnv2_backward_f32's kernels in their shared form.  offset [n,2,h,w] and mask [n,1,h,w]
 * stay compact, and so do grad_offset [n,2,h,w] and grad_mask [n,1,h,w]: the thread that owns a pixel adds the 9 taps' d/dy, d/dx and
 * d/dmask in tap order in registers and stores once, so the 9x-tiled tensors and their gradients never exist (not in the workspace
 * either).  Everything else is crfp_dcnv2_backward_f32's contract: NULL outputs skipped (all five NULL: CRFP_E_BADARG), grad_offset,
 * grad_mask, grad_weight and grad_bias bitwise reproducible, grad_x an atomic sum, argument errors before any HIP call.  Domain: the
 * forward's, cin = cout = 4 (anything else CRFP_E_UNSUPPORTED, size query 0), n <= 65535, h <= 262140, 2^58 tensor elements. */
size_t crfp_dcnv2_shared_backward_workspace_bytes(int n, int c, int h, int w);
int crfp_dcnv2_shared_backward_f32(const float* x, const float* offset, const float* mask, const float* weight, const float* grad_out,
                                   float* grad_x, float* grad_offset, float* grad_mask, float* grad_weight, float* grad_bias,
                                   int n, int cin, int cout, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

/* ---- flow_warp backward: the gradients of crfp_flow_warp_f32's out for a given grad_out[n,c,h,w]: grad_x[n,c,h,w] and
 * grad_flow[n,h,w,2] = (d/dx, d/dy).  The function differentiated is the forward kernel's own: the sample coordinate goes through the
 * same float32 normalisation round trip, border mode clamps it to [0, size - 1] before the floor, and the cell and the four weights are
 * the forward's.  grad_x adds grad_out * weight at each corner inside the plane (the call clears grad_x on `stream` first; a float atomic
 * sum, NOT bitwise reproducible).  grad_flow is the derivative inside the cell the forward's floor picked (the floor's cell at integer
 * positions, as ATen), an invalid corner's value taken as 0, times the chain factor ((size-1)/2) * (2/max(size-1,1)) formed in float32
 * (0 along an axis of size 1), and in border mode times 0 where the unclamped coordinate is <= 0 or >= size - 1; one plain store per
 * element, bitwise reproducible.  A flow that is NaN, infinite or huge has the gradient of the constant the forward computes there:
 * zeros mode adds nothing to grad_x, border mode adds grad_out at the clamped pixel, grad_flow is 0; no address is formed from an
 * unvalidated position.
 * A NULL output is not computed (no clear and no scatter without grad_x); x is read only for grad_flow and may be NULL without it.
 * Both outputs NULL, a NULL flow or grad_out, x NULL with grad_flow wanted, or a size < 1: CRFP_E_BADARG.  padding_mode other than
 * CRFP_PAD_ZEROS / CRFP_PAD_BORDER, n > 65535, h > 262140, w > 2^30 or more than 2^58 tensor elements: CRFP_E_UNSUPPORTED (size query
 * 0).  A missing or short workspace: CRFP_E_WORKSPACE.  Every argument error is returned before any HIP call. */
size_t crfp_flow_warp_backward_workspace_bytes(int n, int c, int h, int w);
int crfp_flow_warp_backward_f32(const float* x, const float* flow, const float* grad_out, float* grad_x, float* grad_flow,
                                int n, int c, int h, int w, int padding_mode, void* workspace, size_t workspace_bytes, void* stream);
/* measurement hook: the same call with the kernel's on-chip summation window of grad_x placed on the pixel tile itself (window = 0)
 * instead of the tile displaced by its centre flow (window = 1, what crfp_flow_warp_backward_f32 does).  Same results up to the order of
 * the atomic sum. */
int crfp_flow_warp_backward_window_f32(const float* x, const float* flow, const float* grad_out, float* grad_x, float* grad_flow,
                                       int n, int c, int h, int w, int padding_mode, int window, void* workspace, size_t workspace_bytes,
                                       void* stream);

/* ---- 3x3 stride-1 pad-1 convolution, NCHW f32, fused bias + activation (fp32 MFMA). */
size_t crfp_conv3x3_workspace_bytes(int n, int cin, int cout, int h, int w);
int crfp_conv3x3_f32(const float* x, const float* weight, const float* bias, float* out, int n, int cin,
                     int cout, int h, int w, int act, float post_scale, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- the conv operator in full: up to two inputs (= conv(torch.cat([x, x2], 1)), e.g. model/CRFP.py:331,1589), optional
 * residual added after activation (model/CRFP.py:48-50 ResidualBlockNoBN), load through pixel_unshuffle(4) (PixelUnShufflePack_v2,
 * model/CRFP.py:28-42: x is [n, cin/16, 4h, 4w]), store into the channel slice [out_c0, out_c0 + cout) of an [n, out_ctotal, h, w]
 * tensor (a fused torch.cat on the output side) or through pixel_shuffle(r), r in {2, 4} (PixelShufflePack, model/CRFP.py:184-193:
 * out is [n, cout/r^2, h r, w r]; no residual, activation none / relu / lrelu).  Pass 0 / 1 for "no shuffle".  fp32 MFMA. */
size_t crfp_conv3x3_ex_workspace_bytes(int n, int cin, int cin2, int cout, int h, int w, int unshuffle_r, int shuffle_r, int has_residual);
int crfp_conv3x3_ex_f32(const float* x, int cin, const float* x2, int cin2, const float* weight, const float* bias, const float* residual,
                        float* out, int n, int cout, int h, int w, int act, float post_scale, int unshuffle_r, int shuffle_r,
                        int out_c0, int out_ctotal, void* workspace, size_t workspace_bytes, void* stream);

/* ---- conv3x3_ex backward: the gradients of crfp_conv3x3_ex_f32's out = act(conv3x3(cat(x, x2)) + bias) * post_scale (+ residual) for a
 * given grad_out (out's shape: [n,cout,h,w], or [n, cout/r^2, h r, w r] with shuffle_r = r > 1): grad_x (x's shape: [n,cin,h,w], or
 * [n, cin/16, 4h, 4w] with unshuffle_r = 4), grad_x2 [n,cin2,h,w], grad_weight [cout, cin + cin2, 3, 3], grad_bias [cout].  The
 * residual's gradient is grad_out itself, so the call takes no residual; a residual combined with an activation has no call site and
 * no backward.  `out` is the forward's saved output, in out's own (shuffled) layout: the activation's derivative is taken from it
 * (relu / lrelu: its sign, which needs post_scale > 0; tanh: 1 - (out/s)^2, sigmoid: (out/s)(1 - out/s), which need post_scale != 0;
 * otherwise CRFP_E_UNSUPPORTED).  The bias is not an input: its gradient is the sum of grad_out * post_scale * act'.
 * Operands: out may be NULL for CRFP_ACT_NONE; x and x2 may be NULL when grad_weight is NULL; weight may be NULL when grad_x and
 * grad_x2 are NULL.  Outputs: a NULL output means "not wanted" and its work is skipped (a NULL grad_x or grad_x2 removes its channels
 * from the input pass, both NULL the pass itself; no weight pass without grad_weight); all four NULL is CRFP_E_BADARG.  Every element of
 * a wanted output is written by the call with a plain store, and the workspace needs no initialisation.
 * Domain: the forward's combination rules (unshuffle_r in {0, 1, 4}, shuffle_r in {0, 1, 2, 4}, ...: CRFP_E_UNSUPPORTED otherwise),
 * cin + cin2 <= 1024, cout <= 1024, n <= 65535, h <= 262140, w <= 2^30, 2^58 tensor elements; beyond it CRFP_E_UNSUPPORTED and the size
 * query returns 0.  A missing required pointer or a size < 1 is CRFP_E_BADARG, a missing or short workspace CRFP_E_WORKSPACE; every
 * argument error is returned before any HIP call.  Asynchronous on `stream`, no host synchronisation.
 * Numbers: fp32 throughout on the exact f32-input MFMA, one rounding per product (no split-fp16: gradients have no bounded range), so
 * scaling grad_out by a power of two scales every gradient by it bit for bit.  Determinism: all four gradients are bitwise reproducible
 * from run to run, whichever subset of them is asked for (no atomics; grad_weight / grad_bias through per-workgroup partial slabs in
 * the workspace added in a fixed order, their count a function of the shape alone). */
size_t crfp_conv3x3_ex_backward_workspace_bytes(int n, int cin, int cin2, int cout, int h, int w, int unshuffle_r, int shuffle_r);
int crfp_conv3x3_ex_backward_f32(const float* x, int cin, const float* x2, int cin2, const float* weight, const float* out,
                                 const float* grad_out, float* grad_x, float* grad_x2, float* grad_weight, float* grad_bias,
                                 int n, int cout, int h, int w, int act, float post_scale, int unshuffle_r, int shuffle_r,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The same two operators with the weight repack hoisted out of the call (pack once per weight update):
 *   crfp_conv3x3_pack_f32 -> crfp_conv3x3_packed_f32           (any cin / cout)
 *   crfp_dcnv2_g8_pack_f32 -> crfp_dcnv2_g8_packed_f32         (cin = cout = 32, deformable_groups = 8, k = 3) */
size_t crfp_conv3x3_packed_bytes(int cin, int cout);
int crfp_conv3x3_pack_f32(const float* weight, const float* bias, int cin, int cout, void* packed, size_t packed_bytes, void* stream);
int crfp_conv3x3_packed_f32(const float* x, const void* packed, float* out, int n, int cin, int cout, int h, int w, int act,
                            float post_scale, void* stream);
size_t crfp_dcnv2_g8_packed_bytes(void);
int crfp_dcnv2_g8_pack_f32(const float* weight, void* packed, size_t packed_bytes, void* stream);
int crfp_dcnv2_g8_packed_f32(const float* x, const float* offset, const float* mask, const void* packed, const float* bias, float* out,
                             int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

/* ---- bilinear resize, align_corners=False, NCHW f32; out = mul * resize(x).  scale_h/scale_w
 * are the source-index scales PyTorch uses (1/scale_factor for nn.Upsample, in/out for size=). */
int crfp_upsample_bilinear_f32(const float* x, float* out, int n, int c, int h, int w, int oh, int ow,
                               float scale_h, float scale_w, float mul, void* stream);

/* bilinear resize with align_corners=True (src = dst * (in - 1) / (out - 1)), NCHW f32; out = mul * resize(x). */
int crfp_upsample_bilinear_ac_f32(const float* x, float* out, int n, int c, int h, int w, int oh, int ow, float mul, void* stream);

/* k x k stride-1 pad-k/2 convolution (k in {3, 5, 7}), NCHW f32, direct fp32 FMA; pre_relu != 0 applies ReLU to the INPUT
 * (the reference's `conv` module, model/CRFP.py:145-152: self.conv(self.act(x))). */
int crfp_convkxk_f32(const float* x, const float* weight, const float* bias, float* out, int n, int cin, int cout, int h, int w,
                     int k, int pre_relu, void* stream);

/* ---- SPyNet.forward(ref, supp) -> flow[n,2,h,w] (model/CRFP.py:698-741), one call.  params: the 60 device pointers of
 * the reference's state_dict order, basic_module.{L}.basic_module.{j}.conv.{weight,bias} for L = 0..5 (coarsest first),
 * j = 0..4 (7x7 convs 8->32->64->32->16->2); the mean / std buffers are the ImageNet constants of :586-591. */
#define CRFP_SPYNET_NUM_PARAMS 60
size_t crfp_spynet_workspace_bytes(int n, int h, int w);
int crfp_spynet_forward(const float* const* params, const float* ref, const float* supp, float* flow, int n, int h, int w,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- sum of squared differences for PSNR: acc[0] += sum((a-b)^2) over [n,c,h,w];
 * acc[1] += the same on the luma the reference's eval computes (24.966*c0+128.553*c1+65.481*c2+16,
 * utils.py:328-330), c==3 only.  acc is 2 doubles (device), zeroed by the caller. */
int crfp_psnr_partial_f32(const float* a, const float* b, double* acc, int n, int c, int h, int w, void* stream);

/* nn.AvgPool2d(2, 2), floor mode (FNet, model/CRFP.py:755): x [n,c,h,w] -> out [n,c,h/2,w/2]. */
int crfp_avgpool2_f32(const float* x, float* out, int n, int c, int h, int w, void* stream);

/* ---- backward of crfp_upsample_bilinear_f32 (scale and size mode, downscaling included): grad_x [n,c,h,w] = the adjoint of the
 * forward applied to grad_out [n,c,oh,ow], times mul.  A gather: every input pixel walks the outputs whose footprint can hold it and
 * keeps those for which the forward's own source-index function names it, with the forward's weight bits; at a clamped edge both
 * weights of an output land on one input and both are added.  An input no output reads gets an exact zero; grad_x needs no clear.
 * fp32, no atomics, bitwise reproducible.  A null pointer, a size < 1 or a scale that is not positive and finite: CRFP_E_BADARG.
 * n * c > 65535, h > 262140, a size above 2^30 or more than 2^58 elements: CRFP_E_UNSUPPORTED.  Refusals precede any HIP call. */
int crfp_upsample_bilinear_backward_f32(const float* grad_out, float* grad_x, int n, int c, int h, int w, int oh, int ow,
                                        float scale_h, float scale_w, float mul, void* stream);

/* backward of crfp_avgpool2_f32: grad_x[y][x] = 0.25 * grad_out[y/2][x/2] inside the pooled area, an exact zero on the odd trailing
 * row / column floor mode drops.  A null pointer, n or c < 1, h or w < 2: CRFP_E_BADARG; the limits above: CRFP_E_UNSUPPORTED. */
int crfp_avgpool2_backward_f32(const float* grad_out, float* grad_x, int n, int c, int h, int w, void* stream);

/* ---- masked Charbonnier loss (loss/loss.py:26-68,115-124) in one pass over pred and target [n,c,h,w]: sums[n][2] (float64, device) =
 * per sample (sum sqrt(d^2 + eps) * w, sum w) with d = pred - target and w the weight expanded over c (1 without a weight: the second
 * sum is then the element count).  weight: NULL with weight_c = 0, [n,1,h,w] with weight_c = 1, or [n,c,h,w] with weight_c = c.
 * Elements in fp32, sums in float64 through per-workgroup partials in the workspace added in a fixed order: bitwise reproducible, no
 * atomics; sums needs no clear.  The backward writes grad_pred = scale[sample] * w * d / sqrt(d^2 + eps); scale is n floats on the
 * device (the upstream gradient of sums[:, 0]).  A null pointer, a size < 1, a weight_c that does not fit, eps negative or not finite:
 * CRFP_E_BADARG.  n > 65535 or more than 2^58 elements: CRFP_E_UNSUPPORTED (size query 0).  A missing or short workspace:
 * CRFP_E_WORKSPACE.  Refusals precede any HIP call. */
size_t crfp_charbonnier_workspace_bytes(int n, int c, int h, int w);
int crfp_charbonnier_f32(const float* pred, const float* target, const float* weight, int weight_c, double* sums, int n, int c, int h,
                         int w, float eps, void* workspace, size_t workspace_bytes, void* stream);
int crfp_charbonnier_backward_f32(const float* pred, const float* target, const float* weight, int weight_c, const float* scale,
                                  float* grad_pred, int n, int c, int h, int w, float eps, void* stream);

/* Fovea fusion + output head of one frame, fused (model/CRFP.py:1672-1684):
 *   f' = conv_tttf(cat(state, x_hr)); new_state = LeakyReLU_0.1(mask ? f' : state); out = conv_last(new_state) + bilinear_x8(lr)
 *   (y_only: + bilinear_x8(0.299 R + 0.587 G + 0.114 B), one channel).
 * state, x_hr, new_state: [n,4,8h,8w]; mask: [n,1,8h,8w] bytes; lr: [n,3,h,w]; out: [n,3|1,8h,8w];
 * w_tttf [4,8,3,3], b_tttf [4], w_last [3|1,4,3,3], b_last [3|1] in the reference's OIHW order. */
size_t crfp_fovea_head_workspace_bytes(int n, int h, int w);
int crfp_fovea_head_f32(const float* state, const float* x_hr, const unsigned char* mask, const float* lr, const float* w_tttf,
                        const float* b_tttf, const float* w_last, const float* b_last, float* new_state, float* out, int n,
                        int h, int w, int y_only, void* workspace, size_t workspace_bytes, void* stream);

/* Masked PSNR + SSIM raw sums in one pass: replaces utils.calc_psnr_and_ssim_cuda -> psnr_cuda / ssim_cuda / _ssim
 * (utils.py:166-185,187-240,242-254; callers trainer.py:349-369, test_video.py:357-369).  a, b: [n,c,h,w] fp32; mask:
 * [n,1,h,w] bytes (0 / non-0) or NULL (= all ones); x' = x*mul + add is the reference's range conversion (1/255, 0 when
 * max-min > 2; 0.5, 0.5 when > 1; else 1, 0).  acc (3 doubles, zeroed by the caller) receives
 * acc[0] += sum m (a'-b')^2 (all channels), acc[1] += sum m SSIM_map (all channels), acc[2] += sum m (per pixel). */
int crfp_psnr_ssim_partial_f32(const float* a, const float* b, const unsigned char* mask, double* acc, int n, int c, int h, int w,
                               float mul, float add, void* stream);

/* Foveated score maps: PSNR and mean SSIM of every k x k window at stride `stride`, each window scored as an image of its own
 * (reference test_video.py:23-63 foveated_metric -> the batch_avg=True branches of utils.py:166-172,197-221,242-254; callers
 * test_video.py:381-384, trainer.py:456,628), fused: no unfold, nothing per window in memory.  hr, sr: [n,c,h,w] fp32; psnr, ssim:
 * [n,Hr,Wr] with Hr = (h-k)/stride + 1, Wr = (w-k)/stride + 1, raw values (dB; the unclipped mean of the SSIM map).  The range
 * conversion of utils.py:244-250 is decided on the device, per image, from the span of `sr` over the pixels some window covers
 * (> 2: x/255; > 1: (x+1)/2), so a batch equals n calls bit for bit and the call never synchronises.  A window with mse == 0 gets
 * -20 log10(sqrt((1/255)^2 / (c k k))) and SSIM 1.  1 <= k <= 16 (CRFP_E_UNSUPPORTED above), k <= h, k <= w, stride >= 1;
 * a null pointer, a bad size or a short workspace is CRFP_E_BADARG.  Each output element is written once (no atomics). */
size_t crfp_window_scores_workspace_bytes(int n);
int crfp_window_scores_f32(const float* hr, const float* sr, float* psnr, float* ssim, int n, int c, int h, int w, int k, int stride,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The eval figures of a batch in one fused pass: for every frame, and for the whole frame (row 0) plus each of m byte masks (rows
 * 1..m; non-zero = inside), PSNR, SSIM, PSNR-Y, SSIM-Y as logged by trainer.py:348-369 and test_video.py:360-370 (utils.py:166-185,
 * 242-254; luma = 24.966 c0 + 128.553 c1 + 65.481 c2 + 16 in fp32 on the channels as they arrive, utils.py:328-330).  sr, hr:
 * [n,c,h,w] fp32; masks: [n,m,h,w] bytes or NULL when m == 0; out: [n,1+m,4] doubles, each written once.  The range conversion of
 * utils.py:244-250 is decided on the device, per frame and separately for RGB (span of hr) and for luma (span of luma(hr)); PSNR is
 * -20 log10(sqrt(se / (msum c))), or -20 log10(sqrt((1/255)^2 / (c h w))) when that mse is 0 (c = 1 for luma), SSIM the masked mean
 * of the 11 x 11 gaussian map.  An empty region is NaN in all four columns (the reference divides by zero there); without
 * CRFP_METRICS_LUMA columns 2 and 3 are NaN.  A batch equals n calls bit for bit; no atomics, no host synchronisation, the workspace
 * needs no initialisation.  Errors: null pointer, n < 1, c outside 1..4, m outside 0..7, null masks with m > 0, LUMA with c != 3
 * (CRFP_E_BADARG); a short or missing workspace (CRFP_E_WORKSPACE).  No lower size limit: a frame smaller than the filter is legal. */
#define CRFP_METRICS_LUMA 1 /* also score luma (c == 3): columns 2 and 3 */
size_t crfp_frame_metrics_workspace_bytes(int n, int m, int h, int w);
int crfp_frame_metrics_f32(const float* sr, const float* hr, const uint8_t* masks, double* out, int n, int c, int m, int h, int w, int flags,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The gaze rig's per-frame inputs from rectangles, one streaming pass (test_video.py:335-358,371-375: the fovea frame and mask, the fovea /
 * outskirt / past regions the metrics score and the regional-DCN box): what a host of crfp_dsv_stream_frame needs to turn a fovea window into
 * that call's full-frame `fv`, `mk` and `fg`, and crfp_frame_metrics_f32's `masks`.  gt, fv: [n,c,h,w] fp32, both given or both NULL (masks
 * only); mk, fg: [n,1,h,w] bytes; regions: [n,3,h,w] bytes, planes fovea, outskirt, past.  rows: DEVICE memory, n rows of
 * CRFP_GAZE_ROW_INTS int32: ints 0..3 the regional box y0, y1, x0, x1 (half-open; the whole frame when there is none), then four entries of
 * five ints y, x, h, w, flags -- entry 0 this frame's fovea window, entries 1..3 the previous frames' windows, newest first; flags bit 0
 * (CRFP_GAZE_EXISTS): the entry exists, bit 1 (CRFP_GAZE_COUNTS): its window counts as mk (the rig: frame index >= fv_start).  With R_e = entry e's rectangle intersected with the frame and G_e = the rectangle grown by `dilate` pixels on all four sides
 * intersected with the frame (the rig's ten 3x3 dilations of one rectangle: dilate = 10; both empty for an entry that does not exist or has
 * h < 1 or w < 1), per pixel p:
 *   fovea = p in R_0;  mk = COUNTS_0 and p in R_0;  outskirt = p in G_0 and not mk;
 *   past = OR over e = 1..3 of (p in G_e and not (COUNTS_e and p in R_e));  fg = p in box;  fv = mk ? gt : +0.
 * Mask bytes are exactly 0 or 1 and every output element is written once.  Rectangles are clipped to the frame on the device in 64-bit
 * arithmetic: no row content addresses outside the planes.  gt is read only inside mk.  16-byte stores when w % 4 == 0 and every pointer is
 * 16-byte aligned, an element-wise form otherwise.  Asynchronous on `stream`, no workspace, no atomics, nothing to initialise.  Errors
 * (CRFP_E_BADARG, before any HIP call): n, c, h, w < 1, dilate < 0, null rows / mk / regions / fg, gt without fv or fv without gt;
 * n > 65535 is CRFP_E_UNSUPPORTED. */
#define CRFP_GAZE_ROW_INTS 24
#define CRFP_GAZE_EXISTS 1
#define CRFP_GAZE_COUNTS 2
int crfp_gaze_prep_f32(const float* gt, const int32_t* rows, float* fv, uint8_t* mk, uint8_t* regions, uint8_t* fg, int n, int c, int h, int w,
                       int dilate, void* stream);

/* 8-bit frame I/O around the fp32 API tensors, two stream kernels (dataset/reds.py:196-203,306,409; test_video.py:100-127,396-410): a host
 * uploads an 8-bit LR frame, a fovea crop and one rectangle, and downloads an 8-bit frame.
 * Ingest.  lr_u8 [n,h,w,3] bytes -> lr [n,3,h,w] fp32, lr[c,y,x] = (float)lr_u8[y,x,c'] / 255.0f with IEEE division, c' = c (2 - c under
 * CRFP_IO_BGR).  crop_u8 [n,fh,fw,3] bytes and rects (DEVICE memory, n rows of CRFP_IO_RECT_INTS int32: y, x, flags, 0; (y, x) = the frame
 * position of the crop's pixel (0, 0)) -> fv [n,3,H,W] fp32, mk [n,1,H,W] bytes: with R = [y, y + fh) x [x, x + fw) intersected with the frame
 * (64-bit arithmetic; empty when bit CRFP_IO_HAS_FOVEA of the row's flags is clear), fv = crop / 255.0f of the matching crop pixel and mk = 1
 * inside R, fv = +0.0f and mk = 0 outside.  A crop may hang over any edge or lie wholly outside.  lr_u8 and lr: both given or both NULL (fovea
 * only); crop_u8, rects, fv, mk: all given or all NULL (LR only).  At most two launches.
 * Export.  sr [n,c,H,W] fp32 -> out_u8 [n,H,W,3] bytes, per channel value (uint8)rintf(fminf(fmaxf(v * 255.0f, 0.0f), 255.0f)): round half to
 * even, NaN gives 0.  c = 3: chroma must be NULL.  c = 1 (a y_only model): chroma [n,3,H,W] RGB fp32 is required and the pixel is, in fp32 with
 * one rounding per operation, u = ((-0.147f r) - (0.289f g)) + (0.436f b), v = ((0.615f r) - (0.515f g)) - (0.100f b) of the chroma pixel,
 * R = y + (1.14f v), G = (y + (-0.396f u)) - (0.581f v), B = y + (2.029f u) with y = sr.  CRFP_IO_BGR swaps the byte order of a pixel.
 * Both: asynchronous on `stream`, no workspace, no atomics, nothing to initialise, every output byte written exactly once; a 4-pixel form when
 * the plane sizes (ingest's fv / mk: W) are multiples of 4, the fp32 pointers 16-byte and the byte pointers (mk, lr_u8, out_u8) 4-byte aligned,
 * an element-wise form otherwise.  Errors (CRFP_E_BADARG, before any HIP call): a half-given group, nothing given, a size < 1, c outside {1, 3},
 * chroma with c = 3 or none with c = 1, unknown flag bits; n > 65535 is CRFP_E_UNSUPPORTED. */
#define CRFP_IO_BGR 1 /* the 8-bit side is B,G,R per pixel (cv2 order) instead of R,G,B */
#define CRFP_IO_RECT_INTS 4
#define CRFP_IO_HAS_FOVEA 1
int crfp_frame_ingest_u8(const uint8_t* lr_u8, const uint8_t* crop_u8, const int32_t* rects, float* lr, float* fv, uint8_t* mk, int n, int h, int w,
                         int fh, int fw, int H, int W, int flags, void* stream);
int crfp_frame_export_u8(const float* sr, const float* chroma, uint8_t* out_u8, int n, int c, int H, int W, int flags, void* stream);

/* Bicubic resize of 8-bit frames, byte for byte what PIL's Image.resize(..., BICUBIC) gives on an 8-bit RGB image (the reference's baseline and
 * y_only chroma frames: test_video.py:241,396-402, dataset/reds.py:281,394,480, trainer.py:331-335).  Integer arithmetic on bytes; only the tap
 * tables are computed in IEEE double.  Per axis with input size I and output size O: scale = I / O, fs = max(scale, 1), support = 2 fs,
 * ksize = (int)ceil(support) * 2 + 1; for output index xx: center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0),
 * cnt = min((int)(center + support + 0.5), I) - xmin, w[x] = f((x + xmin - center + 0.5) / fs) for x < cnt with the a = -0.5 cubic f, divided by
 * their sum in index order unless that is 0, k[x] = (int)(w[x] * 4194304 -+ 0.5) (truncating, sign of w[x]).  A pixel is
 * clamp(((1 << 21) + sum over x < cnt of byte[xmin + x] * k[x]) >> 22, 0, 255) in 32-bit ints with an arithmetic shift.  An image is resampled
 * along x into an 8-bit image [h,W], then along y; channels are independent.  (PIL skips an axis whose size does not change; the taps of such
 * an axis are the identity, so the bytes are the same.)
 * crfp_bicubic_taps: the tables of one axis on the HOST (no GPU call), from the function the device runs: bounds[2 xx] = xmin, bounds[2 xx + 1]
 * = cnt, taps[ksize xx + x] = k[x], zero for x >= cnt.  Returns ksize; CRFP_E_BADARG for a null pointer or a size < 1, CRFP_E_UNSUPPORTED when
 * ksize * out_size does not fit an int, CRFP_E_WORKSPACE when taps_capacity (in ints) < ksize * out_size.
 * crfp_resize_bicubic_u8: src [n,h,w,3] bytes -> dst [n,H,W,3] bytes, or with CRFP_IO_OUT_F32 dst [n,3,H,W] fp32 = (float)byte / 255.0f (IEEE
 * division) of that byte.  crfp_frame_export_y_bicubic_u8: a y_only model's display frame without the fp32 chroma frame -- luma [n,1,H,W] fp32
 * and the LR frame lr_u8 [n,h,w,3] -> out_u8 [n,H,W,3], equal to crfp_frame_export_u8 with c = 1 on chroma = the resized LR frame's bytes / 255.
 * CRFP_IO_BGR: the 8-bit input and the 8-bit output are B,G,R per pixel (the fp32 planes are R,G,B).
 * One call is a table kernel (both axes, one thread per output row or column, into the workspace: no host copy, no synchronisation, so the call
 * can be captured in a graph) and then either one fused launch -- taken when H >= h and W >= w: a workgroup stages the input patch of its 32 x 64
 * output tile in LDS, resamples it along x into LDS and along y into its epilogue (bytes, fp32 planes, or the y_only merge) -- or, for any
 * other geometry, for CRFP_IO_TWO_PASS and for plain resizes only, a kernel along x into an 8-bit image in the workspace and one along y.  The
 * merge exists on the fused path only: another geometry is CRFP_E_UNSUPPORTED and nothing is written.  The workspace (any contents, 16-byte
 * aligned) begins with the tables as int32: bounds of x [2 W], taps of x [ksize_x W], bounds of y [2 H], taps of y [ksize_y H].  Every output
 * byte is written exactly once; no atomics; 4-pixel stores when W % 4 == 0, the fp32 pointers are 16-byte and the byte output 4-byte aligned,
 * one-pixel stores otherwise.  Errors before any HIP call: null pointer, size < 1, unknown flag bits (CRFP_E_BADARG); a short or missing
 * workspace (CRFP_E_WORKSPACE); n > 65535, tables beyond an int or a frame beyond the launch grid (CRFP_E_UNSUPPORTED; the size query gives 0). */
#define CRFP_IO_OUT_F32 2  /* crfp_resize_bicubic_u8: dst is fp32 planar [n,3,H,W] instead of bytes [n,H,W,3] */
#define CRFP_IO_TWO_PASS 4 /* crfp_resize_bicubic_u8: take the two-pass path whatever the geometry (A/B and tests) */
int crfp_bicubic_taps(int in_size, int out_size, int32_t* bounds, int32_t* taps, int taps_capacity);
size_t crfp_resize_bicubic_workspace_bytes(int n, int h, int w, int H, int W);
int crfp_resize_bicubic_u8(const uint8_t* src, void* dst, int n, int h, int w, int H, int W, int flags, void* workspace, size_t workspace_bytes,
                           void* stream);
int crfp_frame_export_y_bicubic_u8(const float* luma, const uint8_t* lr_u8, uint8_t* out_u8, int n, int h, int w, int H, int W, int flags,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- CRFP_DSV engine (mid_channels=32, hr_dcn=True, offset_prop=True; y_only selectable).
 * Parameters arrive as CRFP_DSV_NUM_PARAMS device pointers in the order of the reference's
 * state_dict (weight then bias of each conv, list in crfp_dsv_param_name). */
#define CRFP_DSV_NUM_PARAMS 118
const char* crfp_dsv_param_name(int index);               /* state_dict key of parameter `index` */
int crfp_dsv_param_numel(int index, int y_only);          /* element count of that parameter */
size_t crfp_dsv_packed_weight_bytes(int y_only);
/* repack all parameters into the MFMA / stencil layouts (device -> device, async on stream) */
int crfp_dsv_pack_weights(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);

/* Workspace of a t-frame clip.  A clip call runs the state-independent work of its frames (mask gate, fovea blend, encoder_hr, the upsample
 * conv, the flow up-samplings) as one launch per kernel over a GROUP of frames -- the frames of a clip of up to 8 frames (pairs of frames of a longer one), or the whole clips of a
 * batch while n * t <= 8 -- so the workspace holds one frame slot (x8 frame stack, encoder_hr's two outputs, the upsample conv's output, both
 * up-sampled flows, the gate flags) per frame of a group instead of two per call: t slots for t <= 8; a longer clip goes in groups of two frames
 * with two groups in flight, 4 slots of the tensors the recurrent part reads plus 2 of the launches' temporaries, so that its workspace stays bounded.  One slot (from the layout): 289 MB at h x w = 180 x 320 and 651 MB at
 * 270 x 480 with fp32 storage, 160 MB and 361 MB with bf16 storage; 39 % of it (bf16: 45 %) are the tensors the recurrent part reads.  A 7-frame 180 x 320
 * fp32 clip therefore takes 1.45 GB more than with two slots (bf16: 0.80 GB), a clip of more than 8 frames 0.22 GB more (bf16: 0.14 GB), whatever
 * its length.  The one-frame-per-call workspace (t = 1, the streaming entry points) keeps its two sets and its size. */
size_t crfp_dsv_workspace_bytes(int t, int h, int w);

/* `flags` of the two forward entry points (the round-1 ABI passed y_only in the same slot: 0 / 1 keep their meaning). */
#define CRFP_DSV_Y_ONLY 1     /* the model was built with y_only=True: one output channel */
#define CRFP_DSV_STRICT_F32 2 /* plain fp32 MFMA for every convolution and the DCN GEMM instead of the default split-fp16
                               * scheme (fp32-grade, 3 fp16 MFMAs per product, needs |activation|, |weight| < 65504) */
#define CRFP_DSV_SINGLE_STREAM 4 /* this call enqueues everything on `stream` itself (no fork onto the library's side stream);
                               * same bits, used to measure what the two-stream schedule hides */
#define CRFP_DSV_INPUTS_RESIDENT 8 /* crfp_dsv_stream_frame only.  The caller promises that lr, fv and mk hold their final values when the call
                               * is made (no earlier work on `stream` still writes them) and that they stay untouched until `stream` has
                               * drained this call.  `lr_prev` is ignored (may be NULL): the previous frame is the copy the previous call
                               * on this workspace left inside it, as the reference's model keeps `pre_lrs = lrs.clone()`
                               * (model/CRFP_test.py:2234-2238).  Every call of a sequence, from the `first` one on, must carry the flag and
                               * come from the same host thread (the library keeps a host-side call counter per workspace next to its side
                               * stream).  In return the state-independent part of frame i (FNet, encoder_lr, fovea blend, encoder_hr, the
                               * upsample conv) is enqueued on the side stream WITHOUT waiting for `stream` and runs beside frame i - 1's
                               * recurrent chain (buffer sets alternate with the call parity).  Same bits as without the flag.  Not for
                               * calls under HIP graph capture: the early side-stream work is, by design, not ordered behind `stream`. */

/* Numerics status: a 32-bit word inside the workspace at this byte offset.  Bit 0 is raised (sticky until the next clip
 * / the next `first` streamed frame) when a kernel of the split-fp16 scheme stores a value an fp16 operand cannot hold
 * (|v| >= 65504 or inf); from then on every output frame of the call is filled with NaN instead of plausible garbage.
 * Read it (after synchronising the stream) to tell "overflow" from "NaN inputs", and rerun with CRFP_DSV_STRICT_F32. */
size_t crfp_dsv_status_offset(int t, int h, int w);

/* One clip: lrs[t,3,h,w], fvs[t,3,8h,8w] f32, mks[t,1,8h,8w] u8 (bool), out[t,3|1,8h,8w].
 * Zero initial state; flows from FNet(frame i, frame i-1).  (= crfp_dsv_forward_batch with n = 1.)
 * mks is used as a select (0 / non-0), as the reference's 0 / 1 float mask acts in fvs * mk + x * (1 - mk): fvs is only ever read where mks is set, and the
 * work whose result the select discards (the x8 frame stack, encoder_hr and conv_tttf away from the mask) is skipped per 64 x 16 tile, bit-identically
 * (CRFP_MASK_GATE=0 in the environment launches it densely). */
int crfp_dsv_forward_clip(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                          float* out, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

/* A batch of n independent clips, the reference's own tensor shapes (model/CRFP.py:1510-1535: forward(lrs, fvs, mks) carries the
 * batch axis n through every op; main.py:37-38 scatters batches): lrs[n,t,3,h,w], fvs[n,t,3,8h,8w], mks[n,t,1,8h,8w] u8,
 * out[n,t,3|1,8h,8w].  The n clips walk the recurrent chain in lock-step -- ONE launch per layer and frame step over all n clips --
 * so a 2x-resolution map that is a single round of workgroups for one clip becomes n rounds whose load / MFMA / store phases
 * overlap.  Per clip the arithmetic is that of crfp_dsv_forward_clip: outputs are bit-identical to n one-clip calls.  The workspace
 * holds n recurrent states (query crfp_dsv_batch_workspace_bytes) and n status words at crfp_dsv_batch_status_offset, word b for clip
 * b: an fp16-operand overflow poisons the frames of the clip it happened in and no other, as with one call per clip.  The clip-level stages
 * (FNet, encoder_lr) run once over all n * t frames when n * t <= 32 and in chunks of 8 frames per clip otherwise, so the
 * workspace does not grow with t. */
size_t crfp_dsv_batch_workspace_bytes(int n, int t, int h, int w);
size_t crfp_dsv_batch_status_offset(int n, int t, int h, int w);
int crfp_dsv_forward_batch(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                           float* out, int n, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

/* Streaming: one frame per call, recurrent state kept inside `workspace` (same buffer every call).
 * `first` != 0 resets the state (clear_states of the reference's streaming model). lr_prev may be
 * NULL when first != 0, and is ignored under CRFP_DSV_INPUTS_RESIDENT (the library then keeps the previous frame in the
 * workspace and overlaps the state-independent part of this frame with the previous call's kernels).  fg: optional regional mask [8h,8w] u8 (the reference's `fgs`,
 * model/CRFP_test.py:2296-2298,2361,2375,2389), NULL = all ones. */
int crfp_dsv_stream_frame(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                          const uint8_t* mk, const uint8_t* fg, float* out, int first, int h, int w, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The same for n independent sequences in lock-step, one frame of each per call (the reference's streaming forward carries the batch axis too,
 * model/CRFP_test.py:2250-2451): lr / lr_prev [n,3,h,w], fv [n,3,8h,8w], mk [n,1,8h,8w], out [n,3|1,8h,8w]; the workspace
 * (crfp_dsv_batch_workspace_bytes(n, 1, h, w)) holds the n recurrent states and n status words.  n <= 32; `fg` needs n = 1.  Per sequence the
 * results are bit-identical to n one-sequence call chains.  crfp_dsv_stream_frame = this with n = 1. */
int crfp_dsv_stream_batch(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                          const uint8_t* mk, const uint8_t* fg, float* out, int first, int n, int h, int w, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- CRFP_DSV_CRA engine: the reference's cross-resolution-fusion wiring of the same model (model/CRFP.py:2314-2664; the `_cra` run of
 * eval.sh, factory line main.py:35): CRFP_DSV with the four-level fovea encoder LTE_simple_hr_ps (:156-166) and, after each 2x level's
 * residual block, features <- mk2 * conv_tttf_k(cat(features, fovea level k)) + (1 - mk2) * features with mk2 the x0.25 bilinear resample
 * of the fovea mask (:2501,2533-2535).  mid_channels = 32, hr_dcn = offset_prop = True.  Parameters: CRFP_CRA_NUM_PARAMS device pointers in
 * the order of the reference's CRFP_DSV_CRA state_dict (crfp_cra_param_name).  The forward call takes the tensors, flags, status words and
 * workspace rules of crfp_dsv_forward_batch (n clips in lock-step, bit-identical per clip to n one-clip calls); packed weights and
 * workspaces are this wiring's own (query the crfp_cra_* sizes). */
#define CRFP_CRA_NUM_PARAMS 144
const char* crfp_cra_param_name(int index);
int crfp_cra_param_numel(int index, int y_only);
size_t crfp_cra_packed_weight_bytes(int y_only);
int crfp_cra_pack_weights(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);
size_t crfp_cra_batch_workspace_bytes(int n, int t, int h, int w);
size_t crfp_cra_batch_status_offset(int n, int t, int h, int w);
int crfp_cra_forward_batch(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                           float* out, int n, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
/* Streaming form of the wiring: the reference's one-frame-per-call MRCF_simple_v18_cra (model/CRFP_test.py:2480-2861), i.e. CRFP_DSV_CRA
 * with the state kept between calls.  Arguments, flags (CRFP_DSV_INPUTS_RESIDENT, CRFP_DSV_SINGLE_STREAM, CRFP_DSV_Y_ONLY and -- fp32 entry
 * only -- CRFP_DSV_STRICT_F32), the n <= 32 limit and the status words of crfp_dsv_stream_batch; packed weights are crfp_cra_pack_weights',
 * the workspace is sized by crfp_cra_batch_workspace_bytes(n, 1, h, w) and its status words sit at crfp_cra_batch_status_offset(n, 1, h, w).
 * `fg` is accepted and ignored for any n: the reference's forward takes `fgs` and never reads it.  Streaming a clip one frame per call gives
 * crfp_cra_forward_batch's bits.  The _bf16 twin is declared with the other bf16-storage entry points below. */
int crfp_cra_stream_batch(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                          const uint8_t* mk, const uint8_t* fg, float* out, int first, int n, int h, int w, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- CRFP_simple / CRFP engines: the reference's two ablation wirings in front of CRFP_DSV -- CRFP_simple ("v13", model/CRFP.py:816-1099)
 * and CRFP ("v15", :1101-1385) -- as one-call schedules, for mid_channels 32, or 16 embedded (the Python mirror places the narrower model's
 * parameters inside the 32-channel table at pack time), with hr_dcn = offset_prop = True (round 6; every other constructor combination stays
 * a per-operator composition in the Python mirror).  Against CRFP_DSV: `upsample` keeps all 32 features
 * (:875) and nothing is carried beside a level; the previous state is warped at 8x FIRST and both versions are brought to 2x by
 * `downsample` (:1021-1026); `crfp_dense_*` (the reference's class CRFP) additionally feeds every residual block the warped previous state
 * as a third input (:1311,1316).  Parameters: CRFP_DSV_NUM_PARAMS device pointers under CRFP_DSV's state_dict keys, in its order
 * (crfp_dsv_param_name); `upsample`, `upsample_post` and -- dense -- the four `forward_resblocks_k.main.0` weights have other shapes
 * (crfp_simple_param_numel / crfp_dense_param_numel).  The forward calls take the tensors, flags, status words and workspace rules of
 * crfp_dsv_forward_batch; packed weights and workspaces are each wiring's own. */
int crfp_simple_param_numel(int index, int y_only);
size_t crfp_simple_packed_weight_bytes(int y_only);
int crfp_simple_pack_weights(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);
size_t crfp_simple_batch_workspace_bytes(int n, int t, int h, int w);
size_t crfp_simple_batch_status_offset(int n, int t, int h, int w);
int crfp_simple_forward_batch(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                              float* out, int n, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
int crfp_dense_param_numel(int index, int y_only);
size_t crfp_dense_packed_weight_bytes(int y_only);
int crfp_dense_pack_weights(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);
size_t crfp_dense_batch_workspace_bytes(int n, int t, int h, int w);
size_t crfp_dense_batch_status_offset(int n, int t, int h, int w);
int crfp_dense_forward_batch(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                             float* out, int n, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
/* Streaming forms of the two wirings: the reference's one-frame-per-call MRCF_simple_v13 / MRCF_simple_v15 (model/CRFP_test.py:1184-1486,
 * 1805-2113), i.e. CRFP_simple / CRFP with the state kept between calls.  Arguments, flags (CRFP_DSV_INPUTS_RESIDENT included), the n <= 32
 * limit and the status words of crfp_dsv_stream_batch; packed weights are the wiring's own, the workspace is sized by
 * crfp_{simple,dense}_batch_workspace_bytes(n, 1, h, w) and its status words sit at crfp_{simple,dense}_batch_status_offset(n, 1, h, w).
 * `fg` is accepted and ignored for any n: v13 / v15 compute its resample but never use it (:1357-1359, 1978-1980).  Streaming a clip one
 * frame per call gives the clip call's bits. */
int crfp_simple_stream_batch(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                             const uint8_t* mk, const uint8_t* fg, float* out, int first, int n, int h, int w, void* workspace,
                             size_t workspace_bytes, void* stream);
int crfp_dense_stream_batch(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                            const uint8_t* mk, const uint8_t* fg, float* out, int first, int n, int h, int w, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- bf16 storage (BASELINE configs 3-5): the same engine with every activation tensor and the recurrent state held
 * as bf16 in HBM (half the traffic of the HBM-bound kernels, one bf16 MFMA per product instead of three fp16 ones).
 * What stays fp32: the API tensors (lrs, fvs, out), all accumulators and interpolation arithmetic, biases, and everything
 * that is a coordinate -- flow fields, DCN offsets and masks.  Conv / DCN weights are rounded to bf16 once at pack time.
 * Same arguments as the entry points above; `flags` takes CRFP_DSV_Y_ONLY only.  Packed weights and workspaces are NOT
 * interchangeable between the two builds (query the *_bf16 sizes).  Numerics: see DESIGN.md section 4 (oracle twin that
 * rounds at the same points). */
size_t crfp_dsv_packed_weight_bytes_bf16(int y_only);
int crfp_dsv_pack_weights_bf16(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);
size_t crfp_dsv_workspace_bytes_bf16(int t, int h, int w);
size_t crfp_dsv_status_offset_bf16(int t, int h, int w);
int crfp_dsv_forward_clip_bf16(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                               float* out, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
size_t crfp_dsv_batch_workspace_bytes_bf16(int n, int t, int h, int w);
size_t crfp_dsv_batch_status_offset_bf16(int n, int t, int h, int w);
int crfp_dsv_forward_batch_bf16(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                                float* out, int n, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
int crfp_dsv_stream_frame_bf16(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                               const uint8_t* mk, const uint8_t* fg, float* out, int first, int h, int w, void* workspace,
                               size_t workspace_bytes, void* stream);
int crfp_dsv_stream_batch_bf16(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                               const uint8_t* mk, const uint8_t* fg, float* out, int first, int n, int h, int w, void* workspace,
                               size_t workspace_bytes, void* stream);
size_t crfp_cra_packed_weight_bytes_bf16(int y_only);
int crfp_cra_pack_weights_bf16(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);
size_t crfp_cra_batch_workspace_bytes_bf16(int n, int t, int h, int w);
size_t crfp_cra_batch_status_offset_bf16(int n, int t, int h, int w);
int crfp_cra_forward_batch_bf16(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                                float* out, int n, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
int crfp_cra_stream_batch_bf16(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                               const uint8_t* mk, const uint8_t* fg, float* out, int first, int n, int h, int w, void* workspace,
                               size_t workspace_bytes, void* stream);
size_t crfp_simple_packed_weight_bytes_bf16(int y_only);
int crfp_simple_pack_weights_bf16(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);
size_t crfp_simple_batch_workspace_bytes_bf16(int n, int t, int h, int w);
size_t crfp_simple_batch_status_offset_bf16(int n, int t, int h, int w);
int crfp_simple_forward_batch_bf16(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                                   float* out, int n, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
size_t crfp_dense_packed_weight_bytes_bf16(int y_only);
int crfp_dense_pack_weights_bf16(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);
size_t crfp_dense_batch_workspace_bytes_bf16(int n, int t, int h, int w);
size_t crfp_dense_batch_status_offset_bf16(int n, int t, int h, int w);
int crfp_dense_forward_batch_bf16(const void* packed, int flags, const float* lrs, const float* fvs, const uint8_t* mks,
                                  float* out, int n, int t, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
int crfp_simple_stream_batch_bf16(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                                  const uint8_t* mk, const uint8_t* fg, float* out, int first, int n, int h, int w, void* workspace,
                                  size_t workspace_bytes, void* stream);
int crfp_dense_stream_batch_bf16(const void* packed, int flags, const float* lr, const float* lr_prev, const float* fv,
                                 const uint8_t* mk, const uint8_t* fg, float* out, int first, int n, int h, int w, void* workspace,
                                 size_t workspace_bytes, void* stream);
int crfp_fnet_forward_bf16(const void* packed, const float* cur, const float* prev, float* flow, int n, int h, int w,
                           void* workspace, size_t workspace_bytes, void* stream);
int crfp_dsv_debug_fetch_bf16(const char* name, int t, int h, int w, const void* workspace, float* out_nchw,
                              int* c_out, int* h_out, int* w_out, void* stream);
int crfp_cra_debug_fetch_bf16(const char* name, int t, int h, int w, const void* workspace, float* out_nchw,
                              int* c_out, int* h_out, int* w_out, void* stream);
int crfp_simple_debug_fetch_bf16(const char* name, int t, int h, int w, const void* workspace, float* out_nchw,
                                 int* c_out, int* h_out, int* w_out, void* stream);
int crfp_dense_debug_fetch_bf16(const char* name, int t, int h, int w, const void* workspace, float* out_nchw,
                                int* c_out, int* h_out, int* w_out, void* stream);

/* FNet alone (compute_flow): pairs cur[n,3,h,w], prev[n,3,h,w] -> flow[n,2,h,w] (NCHW). */
int crfp_fnet_forward(const void* packed, const float* cur, const float* prev, float* flow, int n, int h, int w,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-kernel timing for bench.py's roofline object: when enabled every kernel launch is
 * bracketed by hipEvents on its stream; crfp_prof_report synchronises those events and fills
 * up to `cap` records (name, launches, total ms, algorithmic bytes, algorithmic flops). */
typedef struct crfp_prof_record {
    char name[48];
    int launches;
    double total_ms;
    double bytes;
    double flops;
} crfp_prof_record;
int crfp_prof_enable(int on);
int crfp_prof_reset(void);
int crfp_prof_report(crfp_prof_record* out, int cap);
/* diagnostic: how many per-host-thread side-stream tables the fp32 CRFP_DSV engine holds (tables of exited threads are
 * reused by new threads, so a thread-per-request host keeps this at its peak thread count; crfp_shutdown() empties them) */
int crfp_debug_side_tables(void);

/* debug: copy a named intermediate of the last crfp_dsv_* call out of the workspace (Q4 layout
 * converted to NCHW).  Used by the parity tests to bisect; returns CRFP_E_BADARG for unknown names.
 * crfp_cra_ / crfp_simple_ / crfp_dense_debug_fetch read the one-clip workspace of THEIR wiring's forward_batch (each wiring has a
 * layout of its own: 32-channel prop* for simple / dense, the cra.* buffers for cra) under the same contract: out_nchw == NULL returns
 * the item count and fills c / h / w_out.  Frame-slot tensors ("x_hr", "prop0", "flow2", "flow8", "cra.lv0..2", ...) answer to "x" (the
 * last frame of even index) and "x.1" (the last one of odd index). */
int crfp_dsv_debug_fetch(const char* name, int t, int h, int w, const void* workspace, float* out_nchw,
                         int* c_out, int* h_out, int* w_out, void* stream);
int crfp_cra_debug_fetch(const char* name, int t, int h, int w, const void* workspace, float* out_nchw,
                         int* c_out, int* h_out, int* w_out, void* stream);
int crfp_simple_debug_fetch(const char* name, int t, int h, int w, const void* workspace, float* out_nchw,
                            int* c_out, int* h_out, int* w_out, void* stream);
int crfp_dense_debug_fetch(const char* name, int t, int h, int w, const void* workspace, float* out_nchw,
                           int* c_out, int* h_out, int* w_out, void* stream);

/* ---- Test hook: ONE launch of the engines' own 3x3 conv kernels on caller-supplied tensors (tests/test_gpu_conv_probe.py).  Not a product
 * entry: every call builds the plan as the engines do (same source table, same packers, same launchers), converts the API tensors to the
 * build's storage type (fp32, or bf16 for crfp_conv_probe_bf16), launches, converts back, and reports which kernel variant the launcher
 * chose.  All tensors are contiguous fp32 device memory.
 *   src[i]:   CRFP_PROBE_SRC_Q4 [n, nch, h, w] (src_pad = 1: held in padded planes with a zero pad row / column);
 *             CRFP_PROBE_SRC_FLOW2 [n, h, w, 2] (dx, dy), nch = 2;  CRFP_PROBE_SRC_UNSHUF4 [n, nch / 16, 4h, 4w], read as pixel_unshuffle(., 4)
 *   weight [cout, cin, 3, 3], bias [cout] (cin = sum of nch); with weight2 / bias2: rows >= cout_split come from weight2 [cout - cout_split, cin, 3, 3]
 *   out = act(conv + bias) * post_scale (+ residual [n, cout, h, w])
 *   store CRFP_PROBE_ST_Q4: ndst destinations, destination d receives output quads (4 channels each) [dst_q0[d], dst_q1[d]) as
 *             dst[d] [n, min(4 q1, cout) - 4 q0, h, w]; dst_pad[d] = 1: held in padded planes on the device.  Every destination is filled
 *             with 0xFF bytes before the launch, so an element no lane wrote comes back NaN.  dst_raw[d] (optional) receives the raw
 *             destination buffer, n * (q1 - q0) * (h + pad) * (w + pad) * 4 elements of the storage type (dst_f32: float).
 *   store CRFP_PROBE_ST_PS (ps_r in {2, 4}): dst[0] [n, cout / r^2, h r, w r] = pixel_shuffle(out, r)
 *   store CRFP_PROBE_ST_OFFMASK: dst[0] [n, cout, h, w] float; quads < n_off_quads hold 10 tanh(conv) + flow [n, h, w, 2] flipped to (y, x),
 *             the rest sigmoid(conv)
 *   strict: the plain fp32 MFMA (CRFP_DSV_STRICT_F32);  dst_f32: bf16 build, one whole ST_Q4 destination stored as float.
 * mode CRFP_PROBE_SINGLE: conv a.  CRFP_PROBE_DUAL: a and b through launch_conv_mfma_dual.  CRFP_PROBE_PAIR (bf16 build only, else
 * CRFP_E_UNSUPPORTED): a (32 couts, no destination) feeding b (32 -> 32) in one launch; b's source table is ignored.  CRFP_PROBE_PAIR_F32
 * (fp32 build only, else CRFP_E_UNSUPPORTED): the same through the fp32 build's pair kernel (split-fp16 mode).  CRFP_PROBE_S3_CHAIN
 * (fp32 build only): a stores its output only as the pre-split fp16 pair image (a.ndst = 0), b reads it as its single source.
 * status: n words for conv a followed by n words for conv b (device memory, 2 n unsigned): word k is nonzero when batch item k stored a
 * value an fp16 operand cannot hold.  kernel (host memory, 2 ints): CRFP_CONVK_* of conv a and conv b; one launch for both (dual kernel,
 * pair kernel) reports the same value twice; CRFP_CONVK_NONE for an absent conv.  crfp_conv_probe_kernel answers the same question on the
 * host alone (no launch, tensor pointers ignored): *_bf16 for the bf16 build. */
#define CRFP_PROBE_MAX_SRC 4
#define CRFP_PROBE_MAX_DST 3
#define CRFP_PROBE_SRC_Q4 0
#define CRFP_PROBE_SRC_UNSHUF4 2
#define CRFP_PROBE_SRC_FLOW2 3
#define CRFP_PROBE_ST_Q4 0
#define CRFP_PROBE_ST_PS 1
#define CRFP_PROBE_ST_OFFMASK 3
#define CRFP_PROBE_SINGLE 0
#define CRFP_PROBE_DUAL 1
#define CRFP_PROBE_PAIR 2
#define CRFP_PROBE_S3_CHAIN 3
#define CRFP_PROBE_PAIR_F32 4
#define CRFP_CONVK_NONE 0
#define CRFP_CONVK_MFMA_SHIFT_CT2 1 /* conv3x3_mfma_kernel<2, 1, 2> */
#define CRFP_CONVK_MFMA_SHIFT 2     /* conv3x3_mfma_kernel<1, 1, 2> */
#define CRFP_CONVK_MFMA_CT2 3       /* conv3x3_mfma_kernel<2, 1> */
#define CRFP_CONVK_MFMA_ROWS4 4     /* conv3x3_mfma_kernel<1, 1> */
#define CRFP_CONVK_MFMA_ROWS8 5     /* conv3x3_mfma_kernel<1, 2> */
#define CRFP_CONVK_SPLIT8 6         /* conv3x3_split8_kernel */
#define CRFP_CONVK_SPLIT4 7         /* conv3x3_split_kernel<1, 1, 2> */
#define CRFP_CONVK_SPLIT_DUAL 8     /* conv3x3_split_dual_kernel<1, 1, 2> */
#define CRFP_CONVK_BF16_X8 9        /* conv3x3_bf16x8_kernel */
#define CRFP_CONVK_BF16_4W 10       /* conv3x3_bf16_kernel<1> */
#define CRFP_CONVK_BF16_PAIR 11     /* conv3x3_bf16_pair_kernel */
#define CRFP_CONVK_SPLIT_PAIR 12    /* conv3x3_pair_kernel */
typedef struct crfp_probe_conv {
    const float* src[CRFP_PROBE_MAX_SRC];
    const float* weight;
    const float* bias;
    const float* weight2;
    const float* bias2;
    const float* residual;
    const float* flow;
    float* dst[CRFP_PROBE_MAX_DST];
    void* dst_raw[CRFP_PROBE_MAX_DST];
    int nsrc;
    int src_kind[CRFP_PROBE_MAX_SRC], src_nch[CRFP_PROBE_MAX_SRC], src_pad[CRFP_PROBE_MAX_SRC];
    int cout, cout_split, store, ps_r, act, n_off_quads;
    int ndst;
    int dst_q0[CRFP_PROBE_MAX_DST], dst_q1[CRFP_PROBE_MAX_DST], dst_pad[CRFP_PROBE_MAX_DST];
    int strict, dst_f32;
    float post_scale;
} crfp_probe_conv;
size_t crfp_conv_probe_workspace_bytes(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w);   /* 0: refused (crfp_last_error) */
int crfp_conv_probe_kernel(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w, int* kernel);
int crfp_conv_probe(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w, unsigned* status, int* kernel,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t crfp_conv_probe_workspace_bytes_bf16(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w);
int crfp_conv_probe_kernel_bf16(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w, int* kernel);
int crfp_conv_probe_bf16(int mode, const crfp_probe_conv* a, const crfp_probe_conv* b, int n, int h, int w, unsigned* status, int* kernel,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- Test hook: ONE launch of the engines' own 8x narrow conv kernels (csrc/conv_narrow.hip) on caller-supplied tensors
 * (tests/test_gpu_narrow_probe.py).  Not a product entry: every call builds the plans, packs the weights, binds the launch arguments and builds
 * the gate flags as the engines do, converts the API tensors to the build's storage type (fp32, or bf16 for crfp_narrow_probe_bf16), launches,
 * converts back, and reports which kernel the launcher chose and on how many workgroups.  All tensors are contiguous fp32 device memory
 * (mask: bytes).  One crfp_narrow_stencil per 3x3 stencil:
 *   src[i]:   CRFP_PROBE_SRC_Q4 [n, nch <= 4, h, w] or CRFP_PROBE_SRC_FLOW2 [n, h, w, 2] (dx, dy); at most 3 input quads per stencil
 *   src_pad / dst_pad: 0; 1: source 0 / the destination is held in padded planes ((h + 1) x (w + 1), the pad row and column never written);
 *             p > 1: the tensor is a window inside planes p wider and p higher (the regional engine's pitch excess); what surrounds a window
 *             source is filled with non-zero data, what surrounds a window destination keeps the prefill
 *   weight [cout <= 4, cin, 3, 3], bias [cout]; with weight2 / bias2: rows >= cout_split come from weight2 [cout - cout_split, cin, 3, 3]
 *   act CRFP_ACT_NONE / RELU / LRELU01, post_scale, residual [n, 4, h, w]
 *   epi CRFP_NEPI_PLAIN:    dst [n, 4, h, w] = act(conv + bias) * post_scale (+ residual), channels >= cout zero
 *       CRFP_NEPI_BLEND:    dst [n, 4, h, w] = lrelu_0.1(mask ? conv + bias : centre value of source 0); mask [n, 1, h, w] bytes
 *       CRFP_NEPI_LAST:     dst [n, 3 or 1 (y_only), h, w] = conv + bias + x8 bilinear of base_lr [n, 3, h / 8, w / 8] (y_only: its luma); h, w
 *                           multiples of 8; a batch item whose status word is set on entry comes back NaN
 *       CRFP_NEPI_OFFMASK3: dst [n, 4, h, w] = (10 tanh(o0) + flow_y, 10 tanh(o1) + flow_x, sigmoid(o2), 0); flow [n, h, w, 2]
 *   dst2_on:  (plain stencils) dst2 [n, 4, h, w] = lrelu_0.1 of what dst receives, held in padded planes on the device
 *   gate_h:   < 0 dense; 0 .. 3: the mask-gated form, the flag bytes built by launch_mask_gate from `mask` (w a multiple of 4)
 *   dst_raw / dst2_raw (optional): the raw destination buffers, n * (h + pad) * (w + pad) * 4 elements of the storage type (OFFMASK3: float).
 * Every destination is filled with 0xFF bytes before the launch, so an element no lane wrote comes back NaN.
 * mode CRFP_NPROBE_SINGLE: a.  CRFP_NPROBE_PAIR: a feeds b (b brings no source of its own: its one quad is a's output, 4 channels).
 * CRFP_NPROBE_CHAIN: a -> b -> c; res: c adds a's output; c may bring one more global Q4 source.  In a pair or chain only the last stencil
 * has destinations, an epilogue other than PLAIN, or a status word; the launcher's own refusals come back unchanged.
 * status_in (device, n words, may be null = zeros): the range-guard words before the launch; status_out (device, n words): after it; batch
 * item k raises word k.  crfp_narrow_probe_plan fills the report on the host alone (no launch, tensor pointers ignored). */
#define CRFP_NPROBE_SINGLE 0
#define CRFP_NPROBE_PAIR 1
#define CRFP_NPROBE_CHAIN 2
#define CRFP_NEPI_PLAIN 0
#define CRFP_NEPI_BLEND 1
#define CRFP_NEPI_LAST 2
#define CRFP_NEPI_OFFMASK3 3
#define CRFP_NARROWK_NONE 0
#define CRFP_NARROWK_NARROW 1 /* conv3x3_narrow_kernel<kq, epi, gate, st2> */
#define CRFP_NARROWK_SEQ 2    /* conv3x3_narrow_seq_kernel<kq> (fp32 build) */
#define CRFP_NARROWK_PAIR 3   /* conv3x3_narrow_pair_kernel<kq, epi> */
#define CRFP_NARROWK_CHAIN 4  /* conv3x3_narrow_chain_kernel<kq, kqg, res> */
typedef struct crfp_narrow_stencil {
    const float* src[3];
    const float* weight;
    const float* bias;
    const float* weight2;
    const float* bias2;
    const float* residual;
    const float* flow;
    const float* base_lr;
    const unsigned char* mask;
    float* dst;
    void* dst_raw;
    float* dst2;
    void* dst2_raw;
    int nsrc;
    int src_kind[3], src_nch[3];
    int src_pad, dst_pad;
    int cout, cout_split, act, epi, y_only, gate_h, dst2_on;
    float post_scale;
} crfp_narrow_stencil;
typedef struct crfp_narrow_report {
    int kernel;              /* CRFP_NARROWK_* */
    int kq, epi;             /* template arguments: input quads of stencil a, epilogue of the last stencil */
    int gate, st2;           /* conv3x3_narrow_kernel's GATE and ST2 */
    int kqg, res;            /* conv3x3_narrow_chain_kernel's KQG and RES */
    int tiles, workgroups;   /* tiles of the map and workgroups that walk them, per batch item */
} crfp_narrow_report;
size_t crfp_narrow_probe_workspace_bytes(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res,
                                         int n, int h, int w);   /* 0: refused (crfp_last_error) */
int crfp_narrow_probe_plan(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int n, int h,
                           int w, crfp_narrow_report* report);
int crfp_narrow_probe(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int n, int h, int w,
                      const unsigned* status_in, unsigned* status_out, crfp_narrow_report* report, void* workspace, size_t workspace_bytes,
                      void* stream);
size_t crfp_narrow_probe_workspace_bytes_bf16(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c,
                                              int res, int n, int h, int w);
int crfp_narrow_probe_plan_bf16(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int n,
                                int h, int w, crfp_narrow_report* report);
int crfp_narrow_probe_bf16(int mode, const crfp_narrow_stencil* a, const crfp_narrow_stencil* b, const crfp_narrow_stencil* c, int res, int n, int h,
                           int w, const unsigned* status_in, unsigned* status_out, crfp_narrow_report* report, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- Test hook: the fused offset head + DCNv2 launch of a 2x level with the frame's 8x state warp in its idle last-round CUs
 * (tests/test_gpu_dcn_fused_tail.py).  Not a product entry and no conversions: every pointer is a device buffer in the build's storage
 * layout, bound as the clip engine binds it -- feat: the offset feature image (fp32 build: 8 planes [h][w] of 16-byte elements, 8 fp16 each;
 * bf16 build: 8 planes of bf16 quads), wconv / bconv / wdcn / bdcn: the packed images of the head and of dcn_g8, x / warp_src: P4 planes
 * ((h + 1) x (w + 1) quads, zero pad row and column, 8 and 1 of them) behind a zeroed guard of one pad row + one quad, flow [h][w][2],
 * warp_flow [4h][4w][2], out / warp_dst: Q4, status: n words.  Strides between batch items in elements of each tensor's own type.
 * bands = 0: the fused launch, then the stand-alone warp.  bands = k in 1..3: k fused launches, launch b carrying row band b of k of the
 * warp -- unless the launch shape can take no plan (persistent form, full last round), which the report says (plan_taken = 0) and which
 * then runs as bands = 0.  crfp_dcn_tail_plan fills the report on the host alone. */
typedef struct crfp_dcn_tail_args {
    const void *feat, *flow, *wconv, *bconv, *x, *wdcn, *bdcn;
    void* out;
    unsigned* status;
    const void *warp_src, *warp_flow;
    void* warp_dst;
    long long feat_b, flow_b, x_b, out_b, warp_src_b, warp_flow_b, warp_dst_b;
    int n, h, w, bands;
} crfp_dcn_tail_args;
typedef struct crfp_dcn_tail_report {
    int cus;          /* CUs of the device, rounded down to a multiple of 8 */
    int tiles;        /* 8 x 32-pixel tiles of the launch, all batch items */
    int persistent;   /* the launch takes the persistent form (cus workgroups) */
    int warp_wgs;     /* CUs the last round of the one-tile form leaves idle = workgroups of a warp plan; 0: no plan possible */
    int plan_taken;   /* this call's fused launches carry the warp */
    int grid;         /* workgroups of each fused launch */
} crfp_dcn_tail_report;
int crfp_dcn_tail_plan(const crfp_dcn_tail_args* args, crfp_dcn_tail_report* report);
int crfp_dcn_tail_probe(const crfp_dcn_tail_args* args, crfp_dcn_tail_report* report, void* stream);
int crfp_dcn_tail_plan_bf16(const crfp_dcn_tail_args* args, crfp_dcn_tail_report* report);
int crfp_dcn_tail_probe_bf16(const crfp_dcn_tail_args* args, crfp_dcn_tail_report* report, void* stream);

/* ---- Test hook: ONE launch of the engines' own gather kernels (csrc/gather.hip, dcn_fused.inc) on caller-supplied tensors
 * (tests/test_gpu_gather_probe.py).  Not a product entry: every call converts the API tensors (contiguous NCHW fp32 device memory; flow
 * [n, h, w, 2] (dx, dy)) to the build's storage layouts with the library's own conversions, packs the weight images as the engines' pack loop
 * does, binds the launch arguments as the clip engine binds them, launches once, converts back and reports the kernel taken.  Every sampled
 * tensor sits in padded planes ((h + 1) x (w + 1) quads) behind a zeroed guard; every tensor has a batch stride of its own with slack between
 * the items (zero for sources); every destination, its slack included, is filled with 0xFF bytes before the launch.
 *   mode CRFP_GPROBE_WARP:       out [n, c, h, w] = flow_warp(x [n, c, h, w], flow), zeros padding; c in {4, 24, 32}
 *        CRFP_GPROBE_WARP_DUAL:  out [n, 32, h, w], out2 [n, 24, h, w] = flow_warp of x (32) and x2 (24) by one flow field
 *        CRFP_GPROBE_DCN_G8:     out [n, 32, h, w] = DCNv2(x (32), offset = aux [n, 144, h, w] (flow already added), mask [n, 72, h, w], weight
 *                                [32, 32, 3, 3], bias [32]), 8 deformable groups, on the split-fp16 weight image
 *        CRFP_GPROBE_DCN_FUSED:  the same with the offset / mask head inside: aux = the offset feature [n, 32, h, w], head_w [216, 32, 3, 3]
 *                                (rows 0..143 offsets (dy, dx), 144..215 masks), head_b [216]; offsets = 10 tanh + flow (y, x), masks = sigmoid.
 *                                fp32 build: the offset feature reaches the launch as the split-fp16 pair image a centre-tap identity conv
 *                                writes (x to the 22 bits of the pair); bf16 build: as bf16 quads
 *        CRFP_GPROBE_DCN3:       out [n, 4, h, w] = DCNv2 4 -> 4, one group, aux [n, 3, h, w] = (dy, dx, mask) shared by the 9 taps (flow
 *                                already added), weight [4, 4, 3, 3], bias [4]
 *        CRFP_GPROBE_DCN3_FUSED: the same with its 4 -> 3 head inside: aux = the head's input [n, 4, h, w], head_w [3, 4, 3, 3], head_b [3]
 *   out_raw / out2_raw (optional): the raw destination buffers, n * stride elements of the storage type (crfp_gather_report.out_stride /
 *   out2_stride; an item's map is its first elements), slack and the guard behind the last item included.
 *   status (device, n words): the range-guard words after the launch, batch item k raises word k (DCN_G8, DCN_FUSED; zero otherwise).
 * Refused: n outside 1 .. 65535, planes of (h + 1)(w + 1) >= 2^22 elements (the hook's own limit), and DCN_G8 / DCN_FUSED under CRFP_PRECISION=f32.
 * crfp_gather_probe_plan fills the report on the host alone (no launch, tensor pointers ignored). */
#define CRFP_GPROBE_WARP 0
#define CRFP_GPROBE_WARP_DUAL 1
#define CRFP_GPROBE_DCN_G8 2
#define CRFP_GPROBE_DCN_FUSED 3
#define CRFP_GPROBE_DCN3 4
#define CRFP_GPROBE_DCN3_FUSED 5
#define CRFP_GATHERK_NONE 0
#define CRFP_GATHERK_WARP_P4 1         /* flow_warp_p4_kernel */
#define CRFP_GATHERK_WARP_DUAL_SPLIT 2 /* flow_warp_p4_dual_split_kernel<8, 6, 4> */
#define CRFP_GATHERK_WARP_DUAL 3       /* flow_warp_p4_dual_kernel<8, 6, 4> */
#define CRFP_GATHERK_DCN_G8_PIPE 4     /* dcn_g8_pipe_kernel */
#define CRFP_GATHERK_DCN_FUSED 5       /* dcn_fused_kernel<8> */
#define CRFP_GATHERK_DCN_FUSED_PS 6    /* dcn_fused_kernel<8, true> */
#define CRFP_GATHERK_DCN3 7            /* dcn3_kernel<false> */
#define CRFP_GATHERK_DCN3_FUSED 8      /* dcn3_kernel<true> */
typedef struct crfp_gather_args {
    const float *x, *x2, *aux, *mask, *flow;
    const float *head_w, *head_b, *weight, *bias;
    float *out, *out2;
    void *out_raw, *out2_raw;
    unsigned* status;
    int mode, c, n, h, w;
} crfp_gather_args;
typedef struct crfp_gather_report {
    int kernel;                     /* CRFP_GATHERK_* */
    int cus, tiles, persistent;     /* DCN_FUSED: dcn_fused_grid of the launch */
    int split;                      /* WARP_DUAL: the quads of a pixel are split over workgroups */
    int rsv;
    long long out_stride, out2_stride;   /* elements of the storage type between the batch items of the raw destinations */
} crfp_gather_report;
size_t crfp_gather_probe_workspace_bytes(const crfp_gather_args* args);   /* 0: refused (crfp_last_error) */
int crfp_gather_probe_plan(const crfp_gather_args* args, crfp_gather_report* report);
int crfp_gather_probe(const crfp_gather_args* args, crfp_gather_report* report, void* workspace, size_t workspace_bytes, void* stream);
size_t crfp_gather_probe_workspace_bytes_bf16(const crfp_gather_args* args);
int crfp_gather_probe_plan_bf16(const crfp_gather_args* args, crfp_gather_report* report);
int crfp_gather_probe_bf16(const crfp_gather_args* args, crfp_gather_report* report, void* workspace, size_t workspace_bytes, void* stream);

/* ---- The benchmark-only regional wiring, model/CRFP_runtime.py::MRCF_simple_v18.forward(lrs, fvs, warp_size) (:8469-8664;
 * built and timed by the reference's test_runtime.py:41,142) as ONE call per clip.  mid_channels = 32, split_ratio = 3, offset_prop.
 * Same conventions as the CRFP_DSV engine above: parameters as CRFP_RT_NUM_PARAMS device pointers in state_dict order
 * (crfp_rt_param_name), packed once, one workspace, everything enqueued on `stream`.  FNet, the warps and the four DCNs only see the
 * top-left (wp_h, wp_w) window of the 8x frame (multiples of 8, >= 64, inside the frame); fvs is the (fh, fw) fovea crop the
 * reference feeds twice to encoder_hr (:8507) and fuses into the top-left (fh, fw) pixels (:8645-8648).
 * lrs[t,3,h,w], fvs[t,3,fh,fw], out[t,3|1,8h,8w] fp32.  flags: CRFP_DSV_Y_ONLY, CRFP_DSV_SINGLE_STREAM.  Default (split-fp16) precision
 * only: CRFP_DSV_STRICT_F32 is refused.  State kept between calls: three more non-blocking streams + events per (host thread, device)
 * under the same contract as the CRFP_DSV side stream (the three levels of a frame and the next frame's state-independent work run
 * beside the recurrent chain; joined before the call returns; CRFP_SIDE_STREAM=0 / CRFP_DSV_SINGLE_STREAM: none; crfp_shutdown() frees them);
 * the overflow word sits at byte 0 of the workspace and poisons the output like the CRFP_DSV engine's. */
#define CRFP_RT_NUM_PARAMS 158
const char* crfp_rt_param_name(int index);
int crfp_rt_param_numel(int index, int y_only);
size_t crfp_rt_packed_weight_bytes(int y_only);
int crfp_rt_pack_weights(const float* const* params, int y_only, void* packed, size_t packed_bytes, void* stream);
size_t crfp_rt_workspace_bytes(int t, int h, int w, int fh, int fw, int wp_h, int wp_w);   /* 0: bad geometry (crfp_last_error) */
int crfp_rt_forward_clip(const void* packed, int flags, const float* lrs, const float* fvs, float* out, int t, int h, int w,
                         int fh, int fw, int wp_h, int wp_w, void* workspace, size_t workspace_bytes, void* stream);
/* debug (tests and diagnosis only): copy a named intermediate of the last crfp_rt_forward_clip on `workspace` (same geometry) out of it,
 * with the contract of crfp_dsv_debug_fetch: out_nchw == NULL returns the item count and fills c / h / w_out; otherwise Q4 / P4 buffers
 * are converted to NCHW on `stream` (the pad stripped), the [H][W][2] flow fields `flow2` / `flow8` and the split-fp16 images
 * `offfeat0..2` (c = 32: 2 x 4 planes of [H][W] 8 x fp16, x = x0 + x1 * 2^-11) are copied as they are.  Names: flow_lr (t - 1 items, channels
 * 0 and 1 = dx, dy), x_lr, x_hr (t items); of the last frame: state, state_w, prev2, prev2w, carry, carryw, offfeat0..2, aligned0..2,
 * poff, al3, feat2 and its parity set's flow2, flow8, win, upw.  CRFP_E_BADARG (crfp_last_error) for an unknown name, a bad geometry, or a
 * buffer only frames >= 1 write when t = 1. */
int crfp_rt_debug_fetch(const char* name, int t, int h, int w, int fh, int fw, int wp_h, int wp_w, const void* workspace,
                        float* out_nchw, int* c_out, int* h_out, int* w_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
