/* libsr_hip.so — the `upfirdn2d` and `fused_act` extensions of the reference (basicsr/ops/upfirdn2d, basicsr/ops/fused_act),
 * fp32 on gfx950.
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h.  Launch-profiler ids 131-137 (sr_kernel_name); 130 stays unnamed.
 * All kernels are fp32, use no atomics and are bit-reproducible: an output never depends on the tile it falls in, on the
 * plane count or on the batch.  Bad arguments return SR_EINVAL with a message in sr_last_error before anything is launched. */
#ifndef SR_HIP_STYLEGAN2_H
#define SR_HIP_STYLEGAN2_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- upfirdn2d: up-sample, FIR filter, down-sample of independent planes -------------------------------------------------
 *
 * Per plane and per axis (x with in_w, kw, up_x, down_x, pad_x0, pad_x1; y likewise):
 *   1. insert up - 1 zeros after every sample               (length in * up)
 *   2. pad by pad0 in front and pad1 behind; a negative pad crops
 *   3. true convolution with the filter: out'[u] = sum_j P[u + j] * f[k - 1 - j], j = 0 .. k - 1
 *   4. keep every down-th sample: out[o] = out'[o * down]
 * Output size (in * up + pad0 + pad1 - k) / down + 1 (floor), which must be positive.
 *
 * The tensor is the reference kernel's view [major][h][w][minor] with major = n * planes; only minor = 1 (NCHW) is built.
 * Plane c of image i starts at x + i * x_img_stride + c * in_h * in_w (out likewise with the output size), so a channel
 * window of a larger NCHW tensor can be read or written in place.  `filter` is a device pointer to kh * kw floats, row-major.
 *
 * Supported: kh, kw in 1..16, factors in 1..8, minor 1, any pads with a positive output size, (in * up + |pad0| + |pad1| + k)
 * below 2^30 per axis and fewer than 2^31 tiles; addresses are 64-bit.  Everything else is SR_EINVAL.
 *
 * Arithmetic: polyphase.  An output sums only the taps that meet a real sample, at most ceil(kh / up_y) * ceil(kw / up_x), one
 * fmaf each into a zero accumulator, in the order ky ascending, then kx ascending (inserted and padded zeros are never
 * multiplied; a tap that falls outside the image adds a zero product).  |y - exact| <= T * 2^-24 * sum |x| |f| to first order,
 * T the tap count.
 *
 * Instances (sr_upfirdn2d_instance; profiler id 131 + instance):
 *   0  generic           every supported call that is none of the following
 *   1  4x4, up 1, down 1 (both axes)    2  4x4, up 2, down 1    3  4x4, up 1, down 2
 * A workgroup of 256 threads writes a tile of 64 columns x tile_h rows of one plane from a source window staged once in LDS
 * (zero-filled outside the image): tile_h = 32 for instances 1-3; for the generic instance the largest of 32, 16, .. 1 whose
 * window fits 63 KiB. */
int sr_upfirdn2d_f32(const float* x, int64_t x_img_stride, float* out, int64_t out_img_stride, const float* filter, int n,
                     int planes, int in_h, int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                     int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* The dispatch of sr_upfirdn2d_f32 on the host: the instance a call with this filter size and these factors takes (-1 when
 * they are not supported), its tile height and its dynamic LDS bytes (either pointer may be NULL).  The tile width is 64. */
int sr_upfirdn2d_instance(int kh, int kw, int up_x, int up_y, int down_x, int down_y, int* tile_h, size_t* lds_bytes);

/* ---- fused bias + LeakyReLU: cases 30 and 31 of the reference's fused_bias_act kernel -------------------------------------
 *
 * x, ref, out: contiguous [n][c][inner] (the channel is dimension 1 of a tensor of rank >= 2; inner = 1 for [N, C]).
 *   t = x + bias[c]                      (bias may be NULL: no add)
 *   t = s > 0 ? t : t * slope            with s = t, or s = ref when ref is given
 *   y = t * scale
 * One add, one multiply on the negative side, one multiply by scale, each rounded once.  Kernel id 135. */
int sr_fused_bias_act_f32(const float* x, const float* bias, const float* ref, float* out, int n, int c, int64_t inner,
                          float slope, float scale, void* stream);

/* The backward: gx = (out > 0 ? g : g * slope) * scale (the forward with ref = out and no bias) and, from the same pass over
 * g and out, gbias[c] = sum over n and inner of gx; gbias may be NULL (then no workspace is needed and nothing is reduced).
 *
 * Reduction tree (no atomics, fixed order).  A workgroup covers a chunk of 1024 * v values of one (n, c) row, v = 4 when inner
 * is a multiple of 4 and every pointer is 16-byte aligned, else 1.  Each thread adds its 4 * v values in index order
 * (4 * v - 1 additions), a wave adds its 64 lanes in a 6-level tree, thread 0 adds the 4 wave sums in order (3 additions) and
 * writes one partial to the workspace: P = n * ceil(inner / (1024 * v)) partials per channel, ordered by n, then by chunk.  A
 * second launch (kernel id 137) gives each channel one wave: lane l adds partials l, l + 64, ... in order (ceil(P / 64) - 1
 * additions), then the 6-level tree.  A term therefore passes through at most
 *     d = (4 * v - 1) + 6 + 3 + (ceil(P / 64) - 1) + 6 <= 29 + ceil(P / 64)
 * additions, and |gbias - exact| <= d * 2^-24 * sum |gx| to first order.  sr_fused_bias_act_workspace_bytes is the size of the
 * partials at v = 1, the larger of the two (0 for a shape the entry point refuses); SR_ENOSPACE when the workspace is smaller.
 * Kernel id 136 (137 for the second launch). */
size_t sr_fused_bias_act_workspace_bytes(int n, int c, int64_t inner);
int sr_fused_bias_act_bwd_f32(const float* g, const float* out, float* gx, float* gbias, int n, int c, int64_t inner, float slope,
                              float scale, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_STYLEGAN2_H */
