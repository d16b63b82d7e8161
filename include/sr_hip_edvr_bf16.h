/* libsr_hip.so — what the bf16 inference forward of EDVR needs beyond sr_conv3x3_bf16 and the CB16 helpers of sr_hip.h: the
 * modulated deformable conv, a 1x1 conv, the even-position subsample that turns a stride-1 conv into the stride-2 conv, and
 * TSA's pooling, temporal correlation and gate, all on CB16 tensors.  Forward only, gfx950.
 *
 * Declared apart so that sr_hip.h, sr_hip_dcn.h, sr_hip_edvr.h and their ledgers stay as they are; everything here uses the
 * types and status codes of sr_hip.h.  A CB16 tensor is __bf16 [N][C/16][H][W][16]; an image stride is given in elements, is a
 * multiple of 8 and may exceed the image (a channel-block window of a wider tensor); only pixels inside the image are read or
 * written.  Every pointer is 16-byte aligned.  A bad argument returns SR_EINVAL with a message in sr_last_error before anything
 * is launched.  No atomics: every launch is bit-reproducible.  Launch-profiler ids 124-129 (sr_kernel_name); 123 stays unnamed. */
#ifndef SR_HIP_EDVR_BF16_H
#define SR_HIP_EDVR_BF16_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Modulated deformable 3x3 conv (DCNv2), stride 1, pad 1, dilation 1, groups 1; the semantics are those of sr_hip_dcn.h:
 *   y[n][co] = act(bias[co] + sum_{ci,k} W[co][ci][k] * mask[n][9g + k][y][x] * sample_k(x[n][ci])),  g = ci / cpg.
 * Constraint: cin a multiple of 16 and cpg = cin / deformable_groups a multiple of 8.  A sampler item is 8 channels (16 bytes, one
 * half of a 16-channel block) and its group is (16 cb + 8 half) / cpg, so a CB16 block may span two groups (the default
 * network: 64 channels, 8 groups, cpg 8) but a half never does.
 * offset / mask are fp32 NCHW planes, [N][18 dg][H][W] and [N][9 dg][H][W] in the reference's channel order, each with its own
 * image stride in floats: the two parts of what sr_conv3x3_bf16 stores with out_nchw = 1 for a conv of 27 dg couts (mask =
 * offset + 18 dg h w), so offsets keep fp32 resolution.  With mask_is_logit the sampler applies 1 / (1 + expf(-mask)).
 * The sample is the fp32 bilinear value in the reference's operation order times the mask, rounded once to bf16. */
typedef struct sr_dcn_bf16_desc {
  const void* x;             /* CB16, cin channels */
  int64_t x_img_stride;      /* elements between images */
  const float* offset;       /* fp32 NCHW, 18*dg planes */
  int64_t offset_img_stride; /* floats between images */
  const float* mask;         /* fp32 NCHW, 9*dg planes: values, or logits with mask_is_logit */
  int64_t mask_img_stride;
  int mask_is_logit;
  const void* wpacked;       /* mode-0 image of sr_conv3x3_pack_bf16, unchanged */
  const float* bpacked;      /* optional bias image of the same pack call */
  void* out;                 /* CB16, roundup16(cout) channels; every block is written, pad channels as zero */
  int64_t out_img_stride;
  int n, cin, cout, h, w;
  int deformable_groups;
  int ksize, stride, padding, dilation, groups; /* must be 3, 1, 1, 1, 1 */
  float act_slope;           /* LeakyReLU slope of the epilogue; 1 = none */
} sr_dcn_bf16_desc;

/* One fused launch: 4 waves, a tile of 4 rows x 32 columns x 32*COT couts (COT = 2 when roundup32(cout) is a multiple of 64,
 * else 1; the cout groups are the grid's y).  Per 16-channel chunk the sampler writes the LDS column image [9][4][32][32 B]
 * (36 KiB, single-buffered, the half-swap swizzle of conv_bf16.hip) and each wave issues 9*COT v_mfma_f32_32x32x16_bf16 on its
 * row; the weight units (9*COT KiB) are double-buffered LDS-DMA: 54 / 72 KiB, two workgroups per CU.  Kernel id 124. */
int sr_dcn_fwd_bf16(const sr_dcn_bf16_desc* d, void* stream);

/* The instance that launch runs: *cot (1 or 2), *rows (tile rows) and the dynamic LDS bytes it requests (0 for a bad shape). */
size_t sr_dcn_bf16_lds_bytes(int cout, int n, int h, int w, int* cot, int* rows);

/* nn.Conv2d(cin, cout, 1) on CB16: cin a multiple of 16, any cout >= 1, fp32 accumulation on v_mfma_f32_32x32x16_bf16, fp32 bias and
 * LeakyReLU (slope 1 = none), one rounding to bf16.  out has roundup16(cout) channels, pad channels zero.
 *   sr_conv1x1_packed_weight_elems_bf16   bf16 elements of the image wp[group][cin / 16][gc][16] (gc = 64 when roundup32(cout)
 *                                         is a multiple of 64, else 32); 0 for a bad shape
 *   sr_conv1x1_pack_bf16                  OIHW fp32 [cout][cin][1][1] -> that image, bias -> fp32 [roundup32(cout)] (zero padded;
 *                                         sr_conv3x3_packed_bias_floats(cout) floats)
 * The kernel keeps a group's weights in LDS (at most 512 input channels per pass, 64 KiB) and streams 64 pixels per wave straight
 * from memory into the B operand.  Kernel id 125. */
size_t sr_conv1x1_packed_weight_elems_bf16(int cout, int cin);
int sr_conv1x1_pack_bf16(const float* weight, const float* bias, int cout, int cin, void* wpacked, float* bpacked, void* stream);
int sr_conv1x1_bf16(const void* x, int64_t x_img_stride, const void* wpacked, const float* bpacked, void* out,
                    int64_t out_img_stride, int n, int cin, int cout, int h, int w, float act_slope, void* stream);

/* out[n][cb][oy][ox] = x[n][cb][2 oy][2 ox] for an h x w source: (h + 1) / 2 x (w + 1) / 2.  A 3x3 stride-1 pad-1 conv followed by
 * this is the 3x3 stride-2 pad-1 conv exactly.  Kernel id 126. */
int sr_cb16_subsample2_bf16(const void* x, int64_t x_img_stride, void* out, int64_t out_img_stride, int n, int cb, int h, int w,
                            void* stream);

/* MaxPool2d(3, 2, 1) and AvgPool2d(3, 2, 1) of one h x w source in one launch, into two windows of (h + 1) / 2 x (w + 1) / 2.
 * The maximum ignores pad and is exact; the average is the fp32 sum of the nine taps in row-major order (pad counts as 0),
 * divided by 9, rounded once.  Kernel id 127. */
int sr_pool3x3s2_fwd_bf16(const void* x, int64_t x_img_stride, void* out_max, int64_t max_img_stride, void* out_avg,
                          int64_t avg_img_stride, int n, int cb, int h, int w, void* stream);

/* TSA's temporal attention.  emb [b * t][c], emb_ref [b][c], aligned [b * t][c] (CB16, c a multiple of 16).  One thread per
 * (frame, pixel): s = sum_c emb * emb_ref in fp32 with the channels ascending (the products of two bf16 are exact),
 * p = 1 / (1 + expf(-s)), out = bf16(aligned * p) -> CB16 [b * t][c], which read as [b][t * c] is what the fusion convs take.
 * prob: optional fp32 [b * t][h][w] (dense) that receives p.  Kernel id 128. */
int sr_tsa_corr_fwd_bf16(const void* emb, int64_t emb_img_stride, const void* emb_ref, int64_t ref_img_stride, const void* aligned,
                         int64_t aligned_img_stride, float* prob, void* out, int64_t out_img_stride, int b, int t, int c, int h,
                         int w, void* stream);

/* TSA's exit: out = bf16((feat * (1 / (1 + expf(-attn)))) * 2 + attn_add), evaluated in fp32 in that order, on CB16 windows of cb
 * blocks.  Kernel id 129. */
int sr_tsa_gate_fwd_bf16(const void* feat, int64_t feat_img_stride, const void* attn, int64_t attn_img_stride, const void* attn_add,
                         int64_t add_img_stride, void* out, int64_t out_img_stride, int n, int cb, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_EDVR_BF16_H */
