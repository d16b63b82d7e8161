/* libsr_hip.so — the pieces of TOFlow (basicsr/archs/tof_arch.py) that the flow header does not have, fp32 on gfx950: the 9x9
 * convolution of its reconstruction module, the pyramid level input of SPyNetTOF (zeros padding), the 7-frame aligned stack and
 * the residual + denormalise finish.  The 7x7 convolution of the flow header (with the BatchNorm of SPyNetTOF's modules folded
 * into its weights on the host), its 2x2 average pool and its normalisation, and the 1x1 convolution of the RIDNet header serve
 * the rest of the network.
 *
 * Declared apart from sr_hip.h so that the existing ABI headers and their ledgers stay as they are; everything here uses the
 * types and status codes of sr_hip.h.  Launch-profiler ids 188-192 (sr_kernel_name); 187 stays unnamed.
 * Bad arguments return SR_EINVAL with a message in sr_last_error before anything is launched.  Nothing allocates or
 * synchronises.  CB8 is the channel-blocked layout [N][C/8][H][W][8] of sr_hip.h.  Every kernel is bit-reproducible and
 * independent of the batch (image n of a batch gets what a batch of that image alone gets) and uses no atomics. */
#ifndef SR_HIP_TOF_H
#define SR_HIP_TOF_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------ 9x9 convolution ---- */
/* nn.Conv2d(cin, cout, 9, 1, 4) [+ ReLU] on CB8 for the two layers of TOFlow (tof_arch.py:123-124): (cin, cout) = (21, 64),
 * whose source is stored as 24 channels (3 blocks), and (64, 64).  Every other pair is refused.  The pad channels 21-23 of
 * the source never contribute: the kernel replaces them by zero before the multiply, whatever they hold (NaN included).
 *
 * One kernel instance, tof_conv9x9_f32_kernel: an implicit GEMM on v_mfma_f32_32x32x2_f32, 64 couts x (8 rows x 32 columns)
 * per workgroup of 4 waves, the halo'd source tile [16][40][8] and one tap row of weights [9][64][8] staged in LDS per step,
 * both double buffered: 2 * (20 + 18) KiB = 76 KiB, two workgroups per CU.  Any h, w >= 1.
 * Summation order of one output, from a zero accumulator, one fused multiply-add per term: input channel block (8 channels)
 * ascending, tap row ascending, tap column ascending, then within the block the channel pairs (0, 4), (1, 5), (2, 6), (3, 7);
 * zero padding and pad channels contribute exact zeros.  Then + bias, max(., 0) when relu — each one fp32 operation.  With
 * K = 81 * cin_pad terms (cin_pad = 24 or 64),
 *   |out - exact| <= (K + 2) * 2^-24 * (sum |w * x| + |bias|)   to first order.
 *
 * The packed image holds the weights in operand order [cin block][tap row][tap column][64 couts][8 channels] followed by the
 * 64 biases (zeros for a NULL bias): sr_tof_conv9x9_packed_floats(cout, cin) floats in all, 0 for a pair that is not served.
 * Pad channels are zero. */
size_t sr_tof_conv9x9_packed_floats(int cout, int cin);
/* weight: OIHW [cout][cin][9][9]; bias: [cout] or NULL; packed: sr_tof_conv9x9_packed_floats floats, 16-byte aligned.
 * Kernel id 189. */
int sr_tof_conv9x9_pack_f32(const float* weight, const float* bias, int cout, int cin, float* packed, void* stream);

typedef struct sr_tof_conv9x9_desc {
  const float* in;          /* CB8, ceil(cin / 8) blocks at h x w */
  long long in_img_stride;  /* floats between images */
  int cin, cout, n, h, w;
  const float* packed;      /* sr_tof_conv9x9_pack_f32 of the same (cout, cin) */
  float* out;               /* CB8, cout / 8 blocks at h x w */
  long long out_img_stride;
  int relu;                 /* 0 / 1 */
} sr_tof_conv9x9_desc;
/* out must not overlap in.  Pointers 16-byte aligned, image strides multiples of 4 floats, every tensor below 2^31 bytes per
 * image.  Kernel id 188. */
int sr_tof_conv9x9_f32(const sr_tof_conv9x9_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------- level input ---- */
/* The 8-channel input block of one pyramid level of SPyNetTOF (tof_arch.py:86-89) in one launch:
 *   up        = 2 * F.interpolate(flow_prev, scale_factor=2, 'bilinear', align_corners=True)
 *   out       = cat(ref, flow_warp(supp, up, 'bilinear', 'zeros'), up)      3 + 3 + 2 channels = one CB8 block
 *   up_out    = up as a CB8 block (channels 0, 1; the rest 0): what the last conv of the level adds as res1
 * This is the level input of the flow header with the other padding rule; the upsampling coordinate and the warp are the same
 * device functions, so up_out is bit-equal to that launch's and the warped channels are bit-equal to the zeros-padding warp of
 * supp by up.  flow_prev is a CB8 block at (H / 2) x (W / 2) holding the flow in channels 0, 1 (H and W even), or NULL for
 * the coarsest level: up = 0, warp = supp.
 *
 * The N images are N / group groups of `group` pairs, so that the frames are read where they lie.  With n = g * group + k:
 *   ref image  = ref  + g * ref_group_stride                                        [3][H][W]
 *   supp image = supp + g * supp_group_stride + (k + (k >= skip ? 1 : 0)) * 3 * H * W   [3][H][W]
 * A plain batch of pairs is group = 1, skip = 1, both strides 3 * H * W.  The six pairs of a 7-frame clip [b][7][3][H][W]
 * with reference frame r are group = 6, skip = r, ref = clip + r * 3 * H * W, supp = clip, both strides 7 * 3 * H * W.
 * Strides are in floats.  Kernel id 190. */
int sr_tof_level_input_f32(const float* ref, long long ref_group_stride, const float* supp, long long supp_group_stride, int group,
                           int skip, const float* flow_prev, float* out, float* up_out, int N, int H, int W, void* stream);

/* -------------------------------------------------------------------------------------------------- aligned stack ---- */
/* The 21-channel input of conv_1 (tof_arch.py:154-166) in one launch, as a CB8 tensor [b][3][h][w][8]: channels 3i .. 3i + 2
 * hold frame i of the clip warped by its flow ('bilinear', 'zeros': bit-equal to the zeros-padding warp of the flow header on
 * the same frame and flow), or frame ref_idx copied; channels 21-23 are 0.  clip is the normalised [b][7][3][h][w] tensor, read
 * in place.  flows holds the six flows of image n in channels 0, 1 of one-block CB8 tensors at h x w, laid out [b][6]: the
 * flow of frame i of image n is block n * 6 + k, k = i below ref_idx and i - 1 above it, flow_img_stride floats apart
 * (>= 8 * h * w).  Kernel id 191. */
int sr_tof_align_f32(const float* clip, const float* flows, long long flow_img_stride, float* out, long long out_img_stride, int b,
                     int ref_idx, int h, int w, void* stream);

/* --------------------------------------------------------------------------------------------------------- finish ---- */
/* tof_arch.py:170-172: out[n][c] = (y[n][c] + lr_ref[n][c]) * std3[c] + mean3[c] — three fp32 operations in that order,
 * bit-identical to torch on the same operands.  y is the CB8 block conv_4 wrote (channels 0-2), lr_ref the normalised reference
 * frame [3][h][w] of image n at lr_ref + n * lr_img_stride (floats), out is [n][3][h][w]; mean3 / std3 are host arrays.
 * Kernel id 192. */
int sr_tof_finish_f32(const float* y, long long y_img_stride, const float* lr_ref, long long lr_img_stride, float* out, int n, int h,
                      int w, const float* mean3, const float* std3, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_TOF_H */
