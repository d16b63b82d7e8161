/* libsr_hip.so — the entry points of the GFPGANv1OCR plate restorer's StyleGAN2 decoder (gfpganv1_ocr_arch.py and
 * stylegan2_ocr_arch.py of the reference), fp32 inference on gfx950.
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h (CB8 activations [N][C/8][H][W][8], sr_conv3x3_desc, SR_*).  The U-Net half of the network
 * runs on the existing convolutions (sr_conv3x3_f32, sr_convd_f32, sr_conv4x4s2_f32, sr_bilinear2x_fwd_f32, sr_linear_fwd_f32).
 * Launch-profiler ids 91-96 (sr_kernel_name).
 *
 * A StyleConv of the reference computes, per sample n,
 *   s[n, ci]  = latent[n, k] . A[ci]^T / sqrt(nsf) + b[ci]                    (modulation EqualLinear)
 *   d[n, co]  = rsqrt(c^2 sum_ci s[n, ci]^2 Q[co, ci] + 1e-8),  Q = sum_taps W^2, c = 1 / sqrt(cin k^2)
 *   y         = conv(x, c W s[n] d[n])  (+ the blur of the upsampling conv)
 *   out       = lrelu(y + noise_strength * noise + bias, 0.2) * sqrt(2)
 * Here the modulation is never materialised as per-sample weights: the producer of a modulated conv's input writes x * s[n]
 * (the s_next outputs below), the conv runs on the shared weight image, and c * d[n, co] scales its result. */
#ifndef SR_HIP_GFPGAN_H
#define SR_HIP_GFPGAN_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- style coefficients ---- */
/* Every modulated layer of the decoder in ONE launch (one workgroup per layer and sample):
 *   s[n][ci] = (sum_j latent[n][latent_index][j] * mod_w[ci][j]) / sqrt(nsf) + mod_b[ci]
 *   d[n][co] = wscale * rsqrt(wscale^2 * sum_ci s[n][ci]^2 q[co][ci] + 1e-8)   (only when q and d are given)
 * latent element (n, k, j) is at latent[n * latent_img_stride + k * latent_row_stride + j]; row stride 0 repeats one style
 * code for every layer (a 2-D style code).  d carries the weight scale wscale = 1 / sqrt(cin k^2), so a modulated conv
 * multiplies its raw result by d alone.  cin <= 512, nsf <= 1024, n_layers <= SR_GFPGAN_MAX_LAYERS.  Kernel id 91. */
#define SR_GFPGAN_MAX_LAYERS 32
typedef struct sr_gfpgan_style_layer {
  const float* mod_w;  /* [cin][nsf] */
  const float* mod_b;  /* [cin] */
  const float* q;      /* [cout][cin] sum over taps of W^2, or NULL (ToRGB: no demodulation) */
  int cin, cout;
  int latent_index;
  float wscale;
  float* s;            /* [n][cin] out */
  float* d;            /* [n][cout] out, or NULL */
} sr_gfpgan_style_layer;
int sr_gfpgan_style_f32(const float* latent, int64_t latent_img_stride, int64_t latent_row_stride, int nsf,
                        const sr_gfpgan_style_layer* layers, int n_layers, int n, void* stream);

/* NormStyleCode: y[n][j] = x[n][j] * rsqrt(mean_j x[n][j]^2 + 1e-8), rows of `nsf` floats (<= 1024).  y may be x.
 * Kernel id 96. */
int sr_gfpgan_norm_style_f32(const float* x, float* y, int n, int nsf, void* stream);

/* ------------------------------------------------------- modulated convolution tail ---- */
/* The elementwise tail that follows a modulated conv, in the reference's order, on output channel co of sample n at pixel p:
 *   v = raw * demod[n][co]
 *   v = v + noise_strength * noise[n * noise_img_stride + p]       (noise NULL: skipped; stride 0: one map for the batch)
 *   v = lrelu(v + bias[co], act_slope) * alpha                      (FusedLeakyReLU: act_slope 0.2, alpha sqrt(2))
 *   v = v * sft_scale[co - sft_c0] + sft_shift[co - sft_c0]         (co >= sft_c0, only when sft_scale is given; CB8 tensors
 *                                                                    of cout - sft_c0 channels at the output's size)
 *   v = v * s_next[n][co]                                           (only when s_next is given: the next conv's input)
 * demod and s_next are [n][cout] dense.  sft_c0 is a multiple of 8. */
typedef struct sr_gfpgan_tail {
  const float* demod;
  const float* noise;
  int64_t noise_img_stride;
  float noise_strength;
  const float* sft_scale;
  int64_t sft_scale_img_stride;
  const float* sft_shift;
  int64_t sft_shift_img_stride;
  int sft_c0;
  const float* s_next;
} sr_gfpgan_tail;

/* Modulated 3x3 / stride 1 / pad 1 convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32), the implicit GEMM of sr_convd_f32 with
 * the tail above as its epilogue.  base.in is the MODULATED source x * s[n] (CB8, written by its producer); base.wpacked the
 * shared weight image of W [cout][cin][3][3] (sr_convk_pack_f32, ksize 3, mode 0) and base.bpacked the activation bias of
 * the StyleConv packed the same way (required).  Honoured in base: in / in_img_stride / cin_pad / cin_real / in_h / in_w,
 * wpacked / bpacked / cout (multiple of 8), out / out_img_stride, n, act_slope, alpha; every other field must be 0.
 * Kernel id 92; flops = 18 cin cout n h w. */
typedef struct sr_gfpgan_modconv_desc {
  sr_conv3x3_desc base;
  sr_gfpgan_tail tail;
} sr_gfpgan_modconv_desc;
int sr_gfpgan_modconv_f32(const sr_gfpgan_modconv_desc* d, void* stream);

/* The upsampling StyleConv: conv_transpose2d(x * s[n], W^T, stride 2, pad 0) -> (2h+1) x (2w+1), then the FIR blur
 * [1,3,3,1] (x) [1,3,3,1] / 64 * 4 with pad (1, 1) -> 2h x 2w, then the tail.
 *   sr_gfpgan_upconv_f32  polyphase transposed conv on fp32 MFMA: output parity (py, px) of the (2h+1) x (2w+1) map takes the
 *                         taps ky = 1 (py = 1) or ky in {0, 2} (py = 0), likewise kx, so the four parities run 4, 2, 2 and 1
 *                         taps (9 MACs per input pixel, the reference's count).  base as for sr_gfpgan_modconv_f32 with in_h /
 *                         in_w the source size; bpacked, act_slope, alpha and the tail are ignored; out is the raw CB8 map
 *                         of (2 in_h + 1) x (2 in_w + 1).  Kernel id 93; flops = 18 cin cout n h w.
 *   sr_gfpgan_blur_up_f32 the blur and the tail, one thread per 4 channels of a pixel: t CB8 [n][cout][2h+1][2w+1] ->
 *                         out CB8 [n][cout][2h][2w] (h, w: the upconv's source size).  bias is the activation bias [cout]
 *                         (plain).  Kernel id 94. */
int sr_gfpgan_upconv_f32(const sr_gfpgan_modconv_desc* d, void* stream);
int sr_gfpgan_blur_up_f32(const float* t, int64_t t_img_stride, float* out, int64_t out_img_stride, const float* bias,
                          float act_slope, float alpha, const sr_gfpgan_tail* tail, int n, int cout, int h, int w, void* stream);

/* ----------------------------------------------------------------------------- ToRGB ---- */
/* ToRGB (no demodulation): y[n][c][p] = sum_ci (wscale * w[c][ci] * s[n][ci]) x[n][ci][p] + bias[c] + up(skip)[n][c][p] with
 * up = upfirdn2d(skip, [1,3,3,1] (x) [1,3,3,1] / 64 * 4, up 2, pad (2, 1)) of the previous level's image (NULL: none, the 4x4
 * level).  x CB8 of `c` channels (<= 512, multiple of 8) at h x w; w [3][c]; s [n][c]; bias [3]; skip NCHW [n][3][h/2][w/2];
 * y NCHW [n][3][h][w].  x_next (optional, with s_next [n][c]): x_next = x * s_next[n], the modulated input of the next level's
 * upsampling conv, from the same read of x.  Kernel id 95. */
int sr_gfpgan_torgb_f32(const float* x, int64_t x_img_stride, const float* w, float wscale, const float* s, const float* bias,
                        const float* skip, float* y, float* x_next, int64_t x_next_img_stride, const float* s_next, int n, int c,
                        int h, int w_, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_GFPGAN_H */
