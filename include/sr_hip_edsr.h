/* libsr_hip.so — the entry points added for the EDSR generator (edsr_arch.py of the reference), gfx950.
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h (CB8 fp32 activations [N][C/8][H][W][8], CB16 bf16 activations [N][C/16][H][W][16],
 * SR_*).  EDSR's convolutions are sr_conv3x3_f32 / sr_conv3x3_bf16, its fp32 shuffle sr_cb8_pixel_shuffle_f32 and its weight
 * gradients sr_conv3x3_wgrad_f32; what is new is the shuffle of the bf16 path and the image shifts at both ends.
 * Launch-profiler ids 98-100 (sr_kernel_name); id 97 stays unnamed. */
#ifndef SR_HIP_EDSR_H
#define SR_HIP_EDSR_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nn.PixelShuffle(r) of Upsample (arch_util.py:90-109), r in {2, 3}, CB16 bf16 -> CB16 bf16:
 *   dst[n][c][r*h + i][r*w + j] = src[n][c*r*r + i*r + j][h][w]       (torch's channel order, as sr_cb8_pixel_shuffle_f32)
 * src has ceil(r*r*c/16) channel blocks at h x w, dst ceil(c/16) blocks at r*h x r*w; pad channels of dst are written 0.
 * Image strides in bf16 elements, multiples of 8 and not smaller than the image; nothing outside the image is touched.
 * A pure permutation (bit-exact).  One workgroup stages the r*r source blocks of one destination block for 64 pixels of a
 * source row in the LDS, so that both global sides are 16-byte accesses over whole row segments.  h <= 65535 and
 * n * ceil(c/16) <= 65535.  Kernel id 98. */
int sr_cb16_pixel_shuffle_bf16(const void* src, int64_t src_img_stride, void* dst, int64_t dst_img_stride, int n, int c, int h,
                               int w, int r, void* stream);

/* The input shift of EDSR.forward (edsr_arch.py:53), fused with the layout conversion and the channel padding:
 *   dst[n][0][y][x][c] = (x[n][c][y][x] - mean[c]) * range  for c < 3, 0 for the pad channels
 * x NCHW fp32 [n][3][h][w]; dst one channel block per image (CB8 fp32, or CB16 bf16 rounded to nearest even); mean is a HOST
 * pointer to 3 floats.  The subtraction comes before the multiplication, as in the reference.  Kernel id 99. */
int sr_edsr_shift_in_f32(const float* x, float* dst, int64_t dst_img_stride, const float* mean, float range, int n, int h, int w,
                         void* stream);
int sr_edsr_shift_in_bf16(const float* x, void* dst, int64_t dst_img_stride, const float* mean, float range, int n, int h, int w,
                          void* stream);

/* The output shift (edsr_arch.py:59), in place: y[n][c] = y[n][c] / range + mean[c] on NCHW fp32 [n][3][h][w]; mean a HOST
 * pointer to 3 floats, range != 0.  Kernel id 100. */
int sr_edsr_shift_out_f32(float* y, const float* mean, float range, int n, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_EDSR_H */
