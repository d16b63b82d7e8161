/* libsr_hip.so — the entry points of the RIDNet denoiser (ridnet_arch.py of the reference), fp32 on gfx950.
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h (CB8 activations [N][C/8][H][W][8], sr_conv3x3_desc, sr_conv3x3_wgrad_desc, SR_*).
 * Launch-profiler ids 81-90 (sr_kernel_name).
 */
#ifndef SR_HIP_RIDNET_H
#define SR_HIP_RIDNET_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ dilated 3x3 and 1x1 convolution ---- */
/* Stride 1, "same" padding (pad = dilation * (ksize - 1) / 2) convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32), the implicit
 * GEMM of sr_conv3x3_f32 with a halo of `dilation` pixels and taps `dilation` apart:
 *   ksize 3, dilation 1..4   nn.Conv2d(cin, cout, 3, 1, d, d)   (MergeRun, ridnet_arch.py:69-75)
 *   ksize 1, dilation 1      nn.Conv2d(cin, cout, 1)            (EResidualBlockNoBN's last conv), one tap, not a 3x3 of zeros
 * The descriptor is sr_conv3x3_desc plus three fields.  Of `base`, these are honoured: in / in_img_stride / cin_pad / cin_real /
 * in_h / in_w, wpacked / bpacked / cout, out / out_img_stride, n, act_slope, alpha, res1 / res2 / beta1 / beta2 / res_cbn,
 * accumulate, mask_src / mask_img_stride / mask_cb0 / mask_cbn / mask_slope.  upsample, out_nchw, out_h / out_w and the bf16-only
 * fields must be 0.  The output has the input's size; there is no small-map stacking (a dilated tap grid would need `dilation`
 * separator rows between the stacked images).
 *   post_act = 0: out = alpha*act(conv + bias) + beta1*res1 + beta2*res2  (the sr_conv3x3_f32 epilogue, same operation order)
 *   post_act = 1: out = act(alpha*(conv + bias) + beta1*res1 + beta2*res2) (ReLU after the residual add: relu(body(x) + x))
 * then, in both, `accumulate` adds the old destination and mask_src applies the LeakyReLU/ReLU backward, as in sr_conv3x3_f32.
 * out_pre (optional, post_act = 0 only): also stores alpha*act(conv + bias), the value before the residual adds (the
 * aggregation output of MergeRun, whose ReLU mask the backward needs next to the sum).
 * Data gradient: the same call on the mode-1 weight image (flipped and transposed), d->base.in = dY, d->base.cout = the
 * channels of dX.  Weight images: sr_convk_pack_f32 (ksize 3 images are the same as sr_conv3x3_pack_f32's for a dense cin).
 * Kernel ids 81 (ksize 3), 82 (ksize 1); flops = 2 * ksize^2 * cin * cout * n * h * w. */
typedef struct sr_convd_desc {
  sr_conv3x3_desc base;
  int ksize;                /* 1 or 3 */
  int dilation;             /* 1..4 for ksize 3; 1 for ksize 1 */
  int post_act;             /* 1: the activation follows the residual adds */
  float* out_pre;           /* optional CB8 tensor shaped like out: alpha*act(conv + bias) before the residual adds */
  int64_t out_pre_img_stride;
} sr_convd_desc;

size_t sr_convk_packed_weight_floats(int cout, int cin, int ksize, int mode);
/* OIHW weight [cout][cin][k][k] (k = ksize in {1, 3}, dense cin) -> the MFMA image; mode 0 forward (+ bias image of
 * as many floats as sr_conv3x3_packed_bias_floats gives for cout, when bias and bpacked are given), mode 1 data gradient. */
int sr_convk_pack_f32(const float* weight, const float* bias, int cout, int cin, int ksize, int mode, float* wpacked,
                      float* bpacked, void* stream);
int sr_convd_f32(const sr_convd_desc* d, void* stream);

/* Weight / bias gradient of the same convolution:
 *   dweight[co][ci][ty][tx] (+)= scale * sum_{n,y,x} dy[co][y][x] * x[ci][y + d*(ty - r)][x + d*(tx - r)],  r = (ksize - 1) / 2,
 *   dbias[co] (+)= scale * sum dy[co]
 * `base` as for sr_conv3x3_wgrad_f32 with upsample = 0, first_seg = cin, seg = 0 (cin_pad = roundup8(cin)).  A row ring of
 * 2 + d*(ksize-1) source rows per workgroup, partial tiles into the caller's slab, and the fixed-order two-stage reduction of
 * sr_conv3x3_wgrad_f32: no atomics, bit-reproducible.  dweight may point into a FlatAdam arena with accumulate = 1.
 * Kernel ids 83 (ksize 3), 84 (ksize 1). */
typedef struct sr_convd_wgrad_desc {
  sr_conv3x3_wgrad_desc base;
  int ksize;
  int dilation;
} sr_convd_wgrad_desc;

size_t sr_convd_wgrad_slab_bytes(int n, int h, int w, int cout, int cin, int ksize, int dilation);
int sr_convd_wgrad_f32(const sr_convd_wgrad_desc* d, void* stream);

/* ------------------------------------------------------------ the 3-channel ends ---- */
/* MeanShift layers (ridnet_arch.py:8-29): trainable 1x1 convs of 3 channels (a 3x3 mix W plus a bias b).
 *   sr_ridnet_sub_mean_f32      x NCHW [n][3][h][w] -> s CB8 (one block; channels 3..7 written as 0):  s = W x + b.
 *                               Kernel id 85.
 *   sr_ridnet_add_mean_f32      y NCHW = x + W t + b, t = the tail conv's CB8 output (channels 0..2): add_mean plus the
 *                               global residual of RIDNet.forward.  Kernel id 86.
 *   sr_ridnet_sub_mean_bwd_f32  given g = dL/ds (CB8, channels 0..2): dW = sum g x^T, db = sum g (accumulate = 1 adds into
 *                               them; either may be NULL), and, when dx is given, dx = W^T g + dx_res (dx_res NCHW or NULL).
 *   sr_ridnet_add_mean_bwd_f32  given g = dL/dy (NCHW): dW = sum g t^T, db = sum g, and dt = W^T g into a CB8 block
 *                               (channels 3..7 written as 0).
 * The sums run as per-workgroup partials in the caller's workspace (sr_ridnet_mean_workspace_bytes, SR_ENOSPACE when smaller)
 * and a fixed-order finish: bit-reproducible.  Kernel ids 87 (partials + elementwise part), 88 (finish). */
size_t sr_ridnet_mean_workspace_bytes(int n, int h, int w);
int sr_ridnet_sub_mean_f32(const float* x, const float* w, const float* b, float* s, int64_t s_img_stride, int n, int h, int w_,
                           void* stream);
int sr_ridnet_add_mean_f32(const float* x, const float* t, int64_t t_img_stride, const float* w, const float* b, float* y, int n,
                           int h, int w_, void* stream);
int sr_ridnet_sub_mean_bwd_f32(const float* x, const float* g, int64_t g_img_stride, const float* w, float* dw, float* db,
                               int accumulate, float* dx, const float* dx_res, int n, int h, int w_, void* workspace,
                               size_t workspace_bytes, void* stream);
int sr_ridnet_add_mean_bwd_f32(const float* g, const float* t, int64_t t_img_stride, const float* w, float* dw, float* db,
                               int accumulate, float* dt, int64_t dt_img_stride, int n, int h, int w_, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------- streaming helpers ---- */
/* sr_ca_scale_f32       out = u * s[n][c]: RIDNet's channel attention (x * sigmoid(...), no identity, no res_scale), after
 *                       sr_ca_squeeze_f32; out may be u.  Kernel id 89.
 * sr_cb8_relu_mask_f32  out = mask > 0 ? g : slope * g over cbn channel blocks: the ReLU backward where no conv epilogue forms
 *                       the gradient (behind sr_ca_bwd_apply_f32); out may be g.  Kernel id 90. */
int sr_ca_scale_f32(const float* u, int64_t u_img_stride, const float* s, float* out, int64_t out_img_stride, int n, int nf, int h,
                    int w, void* stream);
int sr_cb8_relu_mask_f32(const float* g, int64_t g_img_stride, const float* mask, int64_t mask_img_stride, float slope, float* out,
                         int64_t out_img_stride, int n, int cbn, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_RIDNET_H */
