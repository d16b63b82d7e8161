/* libsr_hip.so — the degradation chain of the reference's plate training set (basicsr/data/ocr_degradation_dataset.py) on the
 * device, fp32 on gfx950: blur (utils/img_process_util.py:filter2D), bilinear resize, Gaussian noise
 * (data/degradations.py:add_gaussian_noise_pt), JPEG (utils/diffjpeg.py:DiffJPEG, forward and backward) and the tail of the
 * dataset's __getitem__ (jitter, gray, round, normalise).
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h.  Launch-profiler ids 141-146 (sr_kernel_name); 140 stays unnamed.
 * All tensors are fp32, NCHW and contiguous.  No kernel uses atomics or scratch, and every result is bit-reproducible: a value
 * never depends on the tile it falls in or on the other samples of the batch.  Bad arguments return SR_EINVAL with a message in
 * sr_last_error before anything is launched.
 *
 * Ragged batches.  A batch whose samples differ in size is a padded buffer [B][C][Hmax][Wmax] plus a device array `sizes` of
 * int32 [B][2] holding (h_i, w_i); NULL means every sample fills the buffer.  The array lives on the device, so the host cannot
 * refuse its contents: a kernel clamps every entry to [0, Hmax] x [0, Wmax] (an entry <= 0 is an empty sample; the Python
 * wrappers refuse both before the upload).  A kernel that writes a ragged tensor writes zero outside each sample's rectangle,
 * so a result never depends on what the buffer held before. */
#ifndef SR_HIP_DEGRADE_H
#define SR_HIP_DEGRADE_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[b][c][y][x] = sum over ky, kx of kernels[kb][ky][kx] * x[b][c][r(y + ky - k/2)][r(x + kx - k/2)], a correlation as
 * F.conv2d and cv2.filter2D compute it, r the reflection that does not repeat the edge pixel (torch 'reflect', cv2's default
 * border).  kernels is [kernel_batch][k][k]; kernel_batch is 1 (kb = 0) or B (kb = b; a sample's channels share its kernel).
 * k odd, 1..21; H > k/2 and W > k/2.  One fmaf per tap into a zero accumulator, ky ascending, then kx ascending:
 * |out - exact| <= (k * k + 1) * 2^-24 * sum |kernel * x| to first order.  out must not overlap x.
 * A workgroup of 256 threads writes 64 columns x 16 rows of one plane from a (16 + k - 1) x (64 + k - 1) source window staged in
 * LDS with the reflection applied while staging; the sample's kernel is in LDS too.  Kernel id 141. */
int sr_filter2d_f32(const float* x, const float* kernels, float* out, int B, int C, int H, int W, int k, int kernel_batch,
                    void* stream);

/* Bilinear size change without antialiasing, half-pixel centres: cv2.resize(INTER_LINEAR) on float images and
 * F.interpolate(mode='bilinear', align_corners=False).  Per axis, with the float32 scale = (float)src_len / (float)dst_len:
 *   s = (d + 0.5f) * scale - 0.5f;  i0 = floor(s);  f = s - i0;  s < 0: i0 = 0, f = 0;  i0 >= src_len - 1: i0 = src_len - 1, f = 0
 * (each a separate float32 operation), i1 = min(i0 + 1, src_len - 1).  The blend
 *   (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c + fx * d)
 * is evaluated in float64 and rounded once: |dst - exact blend| <= 2^-24 * max |x| of the four taps.
 * src is [B][C][Hs][Ws], dst [B][C][Hd][Wd]; src_sizes / dst_sizes are ragged-batch size arrays (either, both or neither); the
 * lengths above are the sample's.  dst is zero outside a sample's rectangle (and everywhere for an empty source).  dst must not
 * overlap src.  Kernel id 142. */
int sr_resize_bilinear_f32(const float* src, const int32_t* src_sizes, float* dst, const int32_t* dst_sizes, int B, int C, int Hs,
                           int Ws, int Hd, int Wd, void* stream);

/* add_gaussian_noise_pt with the draws passed in.  noise is [B][C][H][W] standard normal, noise_gray [B][1][H][W] or NULL,
 * sigma [B] on the 0..255 scale, gray [B] of 0 / 1 (float) or NULL (needs noise_gray when given).  Per value
 *   n = (gray && gray[b] != 0 ? noise_gray[b][0][y][x] : noise[b][c][y][x]) * sigma[b] / 255.f;  out = x + n
 * (multiply, divide, add: three IEEE operations, never contracted), then
 *   clip && rounds: clamp(rintf(out * 255.f), 0, 255) / 255.f;   clip: clamp(out, 0, 1);   rounds: rintf(out * 255.f) / 255.f
 * which is bit-identical to the torch expression.  out may be x.  Kernel id 143. */
int sr_add_gaussian_noise_f32(const float* x, const float* noise, const float* noise_gray, const float* sigma, const float* gray,
                              float* out, int B, int C, int H, int W, int clip, int rounds, void* stream);

/* DiffJPEG.forward for RGB in [0, 1]: x and out are [B][3][H][W], sizes a ragged-batch size array or NULL, factor a device [B]
 * array of quantisation factors (quality_to_factor stays with the caller).  Per sample: pad to a multiple of 16 with zero RGB,
 * * 255, RGB -> YCbCr, 2x2 mean of Cb and Cr, 8x8 DCT of v - 128, divide by table * factor[b], round (rintf, or r + (q - r)^3 when
 * `differentiable`), multiply back, inverse DCT + 128, chroma repeated 2x2, YCbCr -> RGB, clamp to [0, 255], / 255, crop.
 * One workgroup of 256 threads per 16x16 macroblock (four Y blocks, one Cb, one Cr); the DCTs are separable row and column
 * passes in LDS, one fmaf per term in index order.  Pixels inside the sample's rectangle get the result, the rest of the
 * buffer zero.  out may be x.  Kernel id 144. */
int sr_diffjpeg_f32(const float* x, const int32_t* sizes, const float* factor, float* out, int B, int H, int W, int differentiable,
                    void* stream);

/* grad_x = (d out / d x)^T grad_out of sr_diffjpeg_f32 with differentiable = 1 (rintf has no derivative: there is no backward
 * for differentiable = 0).  The quotients and the values before the clamp are recomputed from x; nothing else is saved.  The
 * rounding's derivative is 3 (q - r)^2, the clamp's 1 strictly inside (0, 255) and 0 elsewhere; padding and everything outside a
 * sample's rectangle gets no gradient (grad_x is zero there).  grad_x may be grad_out, not x.  Kernel id 145. */
int sr_diffjpeg_bwd_f32(const float* x, const int32_t* sizes, const float* factor, const float* grad_out, float* grad_x, int B,
                        int H, int W, void* stream);

/* The tail of OCRDegradationDataset.__getitem__ on RGB tensors [B][3][H][W], one pass:
 *   1. jitter ([B][3], or NULL): v = clamp(v + jitter[b][c], 0, 1)
 *   2. gray ([B] of 0 / 1 as float, or NULL) where set: R = G = B = (0.299f * R + 0.587f * G) + 0.114f * B
 *   3. v = clamp(rintf(v * 255.f), 0, 255) / 255.f
 *   4. v = (v - mean3[c]) / std3[c] when mean3 or std3 is given (host arrays of 3 floats; a missing one is 0 resp. 1)
 * Every step is separate IEEE operations.  out may be x.  Kernel id 146. */
int sr_degrade_finish_f32(const float* x, const float* jitter, const float* gray, float* out, int B, int H, int W,
                          const float* mean3, const float* std3, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_DEGRADE_H */
