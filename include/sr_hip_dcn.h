/* libsr_hip.so — modulated deformable convolution (DCNv2), the `dcn` extension of the reference (basicsr/ops/dcn), fp32 on gfx950.
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h (CB8 activations [N][C/8][H][W][8] with image strides and channel-block windows, SR_*).
 * Launch-profiler ids 110-112 (sr_kernel_name); 109 stays unnamed (106-108 are the Winograd kernels).
 *
 * Supported configuration: kernel 3x3, stride 1, padding 1, dilation 1, groups 1, fp32, cin a multiple of 8 and
 * cpg = cin / deformable_groups a multiple of 8 (a CB8 block never straddles two deformable groups: EDVR-M 64/8, EDVR-L 128/8).
 * Everything else returns SR_EINVAL with a message in sr_last_error.
 *
 * Semantics (deform_conv_cuda_kernel.cu:466-497, 571-633 of the reference), tap k = 3i + j, g = ci / cpg:
 *   h_im = y - 1 + i + offset[n][18g + 2k][y][x],  w_im = x - 1 + j + offset[n][18g + 2k + 1][y][x]
 *   sample = 0 unless h_im > -1 && w_im > -1 && h_im < H && w_im < W; inside, the bilinear value of the corners floor / floor + 1
 *            with weights (1-lh)(1-lw), (1-lh)lw, lh(1-lw), lh*lw, each corner counted only when it lies in the image
 *   y[n][co] = act(bias[co] + sum_{ci,k} W[co][ci][i][j] * mask[n][9g + k][y][x] * sample)
 * `offset` (2*9*dg channels) and `mask` (9*dg channels) are separate CB8 pointers with their own image strides, so both can be
 * channel-block windows of one conv_offset output (at dg = 8: blocks [0, 18) and [18, 27) of a 216-channel tensor).  With
 * mask_is_logit the sampler applies 1 / (1 + expf(-mask)), so DCNv2Pack needs no sigmoid pass and no copy. */
#ifndef SR_HIP_DCN_H
#define SR_HIP_DCN_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sr_dcn_desc {
  const float* x;            /* CB8, cin channels */
  int64_t x_img_stride;      /* floats between images */
  const float* offset;       /* CB8, 18*dg channels in the reference's order */
  int64_t offset_img_stride;
  const float* mask;         /* CB8, 9*dg channels: values, or logits with mask_is_logit */
  int64_t mask_img_stride;
  int mask_is_logit;
  const float* wpacked;      /* forward image of sr_convk_pack_f32 (ksize 3, mode 0) or sr_conv3x3_pack_f32, unchanged */
  const float* bpacked;      /* optional bias image of the same pack call */
  float* out;                /* CB8, roundup8(cout) channels; every block is written */
  int64_t out_img_stride;
  int n, cin, cout, h, w;
  int deformable_groups;
  int ksize, stride, padding, dilation, groups; /* must be 3, 1, 1, 1, 1 */
  float act_slope;           /* LeakyReLU slope of the epilogue; 1 = none */
} sr_dcn_desc;

/* The hot path, one fused launch: convd_f32_kernel's workgroup (4 waves, 32*COT couts x 4*PT rows x 32 columns,
 * v_mfma_f32_32x32x2_f32) with the X staging replaced by a sampler that writes, per tap, the masked bilinear value of the
 * chunk's 8 channels into the LDS column image [9][4*PT][32][8] (36 KiB at 4 rows, 72 KiB at 8; single-buffered) next to the
 * double-buffered LDS-DMA weight units (9 / 18 KiB each): 108 KiB at most of the 160 KiB.  8-row tiles, 4-row tiles when the
 * launch would not cover the chip once (the rule of sr_convd_f32).  Bit-reproducible.  Kernel id 110. */
int sr_dcn_fwd_f32(const sr_dcn_desc* d, void* stream);

/* The masked columns as a CB8 tensor of 9*cin channels, tap-major (channel = k*cin + ci), image stride 9*cin*h*w: uses x,
 * offset, mask and the geometry of `d`.  sr_convd_wgrad_f32 with ksize 1 on (cols, dy) then gives dweight as [cout][9*cin] and
 * dbias with its fixed-order reduction; sr_convd_f32 with ksize 1 on cols is the alternative forward.  SR_ENOSPACE when
 * cols_bytes < sr_dcn_cols_bytes.  Kernel id 111. */
size_t sr_dcn_cols_bytes(int n, int cin, int h, int w);
int sr_dcn_cols_f32(const sr_dcn_desc* d, float* cols, size_t cols_bytes, void* stream);

/* Weight images of the two ksize-1 GEMMs around the columns.
 *   sr_dcn_pack_t_f32          OIHW [cout][cin][3][3] -> the sr_convd_f32 ksize-1 forward image of Wt[k*cin + ci][co], so that
 *                              dcol = Wt * dy (9*cin output channels from roundup8(cout) input channels)
 *   sr_dcn_weight_unpack_f32   [cout][9*cin] (tap-major, what the ksize-1 weight gradient writes) -> OIHW [cout][cin][3][3];
 *                              accumulate = 1 adds into dweight */
size_t sr_dcn_packed_t_weight_floats(int cout, int cin);
int sr_dcn_pack_t_f32(const float* weight, int cout, int cin, float* wpacked, void* stream);
int sr_dcn_weight_unpack_f32(const float* dw_cols, int cout, int cin, float* dweight, int accumulate, void* stream);

/* Scatter and coordinate gradients from dcol = Wt * dy (CB8, 9*cin channels tap-major, image stride 9*cin*h*w).  `fwd` gives x,
 * offset, mask, mask_is_logit and the geometry.  Any of dx / doffset / dmask may be NULL (that work is skipped); doffset and
 * dmask are given and omitted together.
 *   doffset, dmask  a gather: one thread per (image, group, tap, pixel) sums its cpg channels in channel order, so both are
 *                   bit-reproducible.  With mask_is_logit dmask is the logit gradient dmask * m * (1 - m), and both land
 *                   directly in the two windows of the conv_offset output's gradient.  Pad channels are not written.
 *   dx              scattered with atomicAdd(float*) into the caller's ZEROED tensor, as the reference does: the one gradient
 *                   of this library whose last bits depend on arrival order (4 corners x 9 taps x cin adds of 4 bytes per
 *                   output pixel).
 * Outside the `inside` test all three contributions are zero (the reference's weights).  Kernel id 112. */
typedef struct sr_dcn_bwd_desc {
  sr_dcn_desc fwd;
  const float* dcol;
  float* dx;
  int64_t dx_img_stride;
  float* doffset;
  int64_t doffset_img_stride;
  float* dmask;
  int64_t dmask_img_stride;
} sr_dcn_bwd_desc;

int sr_dcn_bwd_data_f32(const sr_dcn_bwd_desc* d, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_DCN_H */
