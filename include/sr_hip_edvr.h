/* libsr_hip.so — what EDVR (basicsr/archs/edvr_arch.py of the reference) needs beyond the convolutions, the deformable conv
 * and the resamplers the library already has: a stride-2 3x3 conv, the zero insertion its backward runs on, TSA's two poolings
 * in one pass, TSA's temporal correlation and its final gate.  fp32 on gfx950.
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h (CB8 activations [N][C/8][H][W][8] with image strides and channel-block windows, SR_*).
 * Launch-profiler ids 114-122 (sr_kernel_name); 113 stays unnamed.  No atomics: every launch is bit-reproducible. */
#ifndef SR_HIP_EDVR_H
#define SR_HIP_EDVR_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sr_conv3x3s2_desc {
  const float* in;           /* CB8, cin_pad channels, in_h x in_w */
  int64_t in_img_stride;     /* floats between images */
  int cin_pad;               /* a multiple of 8; pad channels meet zero weights */
  int in_h, in_w;
  const float* wpacked;      /* forward image of sr_convk_pack_f32 (ksize 3, mode 0) or sr_conv3x3_pack_f32 (mode 0), unchanged */
  const float* bpacked;      /* optional bias image of the same pack call */
  int cout;
  float* out;                /* CB8, roundup8(cout) channels, (in_h + 1) / 2 x (in_w + 1) / 2; every block is written */
  int64_t out_img_stride;
  int n;
  float act_slope;           /* LeakyReLU slope of the epilogue; 1 = none */
} sr_conv3x3s2_desc;

/* y = lrelu(bias + conv(x)), 3x3, stride 2, pad 1: y[oy][ox] = sum W[ty][tx] x[2 oy - 1 + ty][2 ox - 1 + tx], for any
 * in_h, in_w >= 1.  The implicit GEMM of sr_convd_f32 (4 waves, 32 * COT couts x 4 * PT output rows x 32 output columns on
 * v_mfma_f32_32x32x2_f32, LDS-DMA staging, double-buffered 8-channel chunks); the staged source tile is [2 * TH + 1][65][8] with
 * the even and the odd source columns of a row in separate planes, so a tap's 32 lanes read 32 consecutive pixels of one plane
 * (conflict-free, as the stride-1 kernels).  8-row tiles, 4-row tiles when the launch would not cover the chip once (the rule
 * of sr_convd_f32, on the output size).  Kernel id 114. */
int sr_conv3x3s2_f32(const sr_conv3x3s2_desc* d, void* stream);

/* The dynamic LDS bytes the launch of sr_conv3x3s2_f32 requests for this cout, batch and source size (0 for a bad shape):
 * 2 * (roundup1024((2 * 4 PT + 1) * 65 * 32) + 9 * COT * 1024) for the instance (COT, PT) the dispatch rule picks. */
size_t sr_conv3x3s2_lds_bytes(int cout, int n, int in_h, int in_w);

/* out[n][cb][y][x] = (y, x both even) ? dy[n][cb][y / 2][x / 2] : 0 for an h x w `out`; dy is (h + 1) / 2 x (w + 1) / 2.
 * The stride-2 conv is the stride-1 conv sampled at even positions, so its data gradient is sr_conv3x3_f32 (mode-1 image) and
 * its weight gradient sr_conv3x3_wgrad_f32 on this tensor, both exact (the added products are zeros).  Kernel id 115. */
int sr_cb8_zero_insert2_f32(const float* dy, int64_t dy_img_stride, float* out, int64_t out_img_stride, int n, int cb, int h,
                            int w, void* stream);

/* MaxPool2d(3, 2, 1) and AvgPool2d(3, 2, 1) (count_include_pad: always / 9, pad counts as 0; the maximum ignores pad) of one
 * h x w source in one launch, into two windows of (h + 1) / 2 x (w + 1) / 2: the torch.cat([max, avg], 1) the next conv reads
 * when both are windows of one tensor.  The average is the row-major sum of the nine taps divided by 9.  Kernel id 116. */
int sr_pool3x3s2_fwd_f32(const float* x, int64_t x_img_stride, float* out_max, int64_t max_img_stride, float* out_avg,
                         int64_t avg_img_stride, int n, int cb, int h, int w, void* stream);

/* The adjoint, gather form: each source pixel visits the up to 4 windows that cover it in (oy, ox) order, recomputes the
 * window's arg-max (the first maximal element in row-major order, as torch's CPU max_pool2d) and adds g_max when it is that
 * element, then g_avg / 9.  No index tensor.  Kernel id 117. */
int sr_pool3x3s2_bwd_f32(const float* x, int64_t x_img_stride, const float* g_max, int64_t gmax_img_stride, const float* g_avg,
                         int64_t gavg_img_stride, float* dx, int64_t dx_img_stride, int n, int cb, int h, int w, void* stream);

/* TSA's temporal attention (edvr_arch.py:151-163).  emb [b * t][c], emb_ref [b][c], aligned [b * t][c] (CB8, c a multiple of
 * 8, h x w).  One thread per (frame, pixel): s = sum_c emb * emb_ref with the channels in ascending order in one lane (c
 * rounded products, c adds, the first of them onto 0 and exact), p = 1 / (1 + expf(-s)) -> prob [b * t][h][w] (dense), out = aligned * p -> CB8
 * [b * t][c], which read as [b][t * c] is the tensor the fusion convs take.  Kernel id 118. */
int sr_tsa_corr_fwd_f32(const float* emb, int64_t emb_img_stride, const float* emb_ref, int64_t ref_img_stride,
                        const float* aligned, int64_t aligned_img_stride, float* prob, float* out, int64_t out_img_stride, int b,
                        int t, int c, int h, int w, void* stream);

/* Its adjoint given g = d out: d_aligned = g * p; ds = (sum_c g * aligned, channels ascending in one lane) * (p * (1 - p)) ->
 * `dcorr` [b * t][h][w] (dense; the caller's scratch, kept as the correlation's gradient); d_emb = ds * emb_ref (kernel id
 * 119); d_emb_ref = sum_t ds_t * emb_t with t ascending from 0 (kernel id 120). */
int sr_tsa_corr_bwd_f32(const float* g, int64_t g_img_stride, const float* emb, int64_t emb_img_stride, const float* emb_ref,
                        int64_t ref_img_stride, const float* aligned, int64_t aligned_img_stride, const float* prob, float* dcorr,
                        float* d_aligned, int64_t da_img_stride, float* d_emb, int64_t de_img_stride, float* d_emb_ref,
                        int64_t dr_img_stride, int b, int t, int c, int h, int w, void* stream);

/* TSA's exit: out = (feat * m) * 2 + attn_add with m = 1 / (1 + expf(-attn)) (kernel id 121), and its adjoint d_feat = g * (2 m),
 * d_attn = ((g * feat) * 2) * (m * (1 - m)) (kernel id 122); d attn_add is g itself.  All operands are CB8 windows of cb blocks. */
int sr_tsa_gate_fwd_f32(const float* feat, int64_t feat_img_stride, const float* attn, int64_t attn_img_stride,
                        const float* attn_add, int64_t add_img_stride, float* out, int64_t out_img_stride, int n, int cb, int h,
                        int w, void* stream);
int sr_tsa_gate_bwd_f32(const float* g, int64_t g_img_stride, const float* feat, int64_t feat_img_stride, const float* attn,
                        int64_t attn_img_stride, float* d_feat, int64_t df_img_stride, float* d_attn, int64_t da_img_stride, int n,
                        int cb, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_EDVR_H */
