/* libsr_hip.so — RCAN's channel attention on CB16 bf16 activations (forward only), gfx950.
 *
 * The bf16 twins of sr_hip.h's sr_ca_squeeze_f32 and sr_ca_excite_f32, declared apart so that the existing ABI headers and their
 * ledgers stay as they are; everything here uses the types and status codes of sr_hip.h.  Tensors are CB16
 * (__bf16 [N][nf/16][H][W][16], 32-byte pixels); image strides are in bf16 elements, multiples of 8, and may exceed the image:
 * only pixels inside the images are read or written.  The pooled means, the MLP and its fp32 parameters, and the gates s are
 * fp32.  No atomics: every launch is bit-reproducible.  Launch-profiler ids 102-104 (sr_kernel_name); id 101 stays unnamed. */
#ifndef SR_HIP_CA_BF16_H
#define SR_HIP_CA_BF16_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace sr_ca_squeeze_bf16 needs: one fp32 partial sum per (image, channel, band of 2048 pixels), rounded up
 * to 64 floats.  0 for a shape the squeeze refuses. */
size_t sr_ca_workspace_bytes_bf16(int n, int nf, int hid, int h, int w);

/* The squeeze of ChannelAttention (rcan_arch.py:8-24) on the CB16 tensor u (all nf channels):
 *   p[n][c] = mean_hw u[n][c],  h = relu(W1 p + b1),  s = sigmoid(W2 h + b2)
 * w1 [hid][nf], b1 [hid], w2 [nf][hid], b2 [nf]: the fp32 1x1 conv parameters as stored (not rounded to bf16).  p [n][nf] and
 * hbuf [n][hid] may be NULL; s [n][nf] is required.  bf16 -> fp32 is exact, so the sums are fp32 sums of the stored values:
 * one workgroup per (image, channel block, band) writes 16 partials (each lane loads 16-byte halves of pixels, 8 per lane;
 * a fixed butterfly within the wave, then the waves in order), and one workgroup per image sums the bands in band order and
 * runs the MLP with its dot products in channel order.
 * SR_EINVAL: nf not a multiple of 16 or above 512, hid outside [1, nf], n, h or w below 1, a NULL required pointer, u not
 * 16-byte aligned, an image stride below the image; SR_ENOSPACE: workspace below sr_ca_workspace_bytes_bf16.  Kernel ids 102
 * (partials), 103 (finish). */
int sr_ca_squeeze_bf16(const void* u, int64_t u_img_stride, int n, int nf, int h, int w, const float* w1, const float* b1,
                       const float* w2, const float* b2, int hid, float* p, float* hbuf, float* s, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The excite and the residual of the RCAB (rcan_arch.py:27-46) in one streaming pass:
 *   out = bf16(x + res_scale * (u * s[n][c]))
 * evaluated in fp32 in that order and rounded once, to nearest even.  x, u, out CB16 of nf channels; out may be x (in place);
 * s [n][nf] fp32, 16-byte aligned.  One 16-byte load per source and one 16-byte store per half pixel.  Refusals as the
 * squeeze's.  Kernel id 104. */
int sr_ca_excite_bf16(const void* x, int64_t x_img_stride, const void* u, int64_t u_img_stride, const float* s, void* out,
                      int64_t out_img_stride, int n, int nf, int h, int w, float res_scale, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_CA_BF16_H */
