/* libsr_hip.so — optical flow building blocks, fp32 on gfx950: flow warping (basicsr/archs/arch_util.py:112-143, flow_warp)
 * and the pieces of SpyNet (basicsr/archs/spynet_arch.py): the 7x7 convolution of its basic modules, the per-level input
 * block and the image pyramid.
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h.  Launch-profiler ids 148-157 (sr_kernel_name); 147 stays unnamed.
 * Bad arguments return SR_EINVAL with a message in sr_last_error before anything is launched.  CB8 is the channel-blocked
 * layout [N][C/8][H][W][8] of sr_hip.h.  Every kernel but the dx scatter of sr_flow_warp_bwd_f32 is bit-reproducible and
 * independent of the batch: image n of a batch gets what a batch of that image alone gets. */
#ifndef SR_HIP_FLOW_H
#define SR_HIP_FLOW_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------ 7x7 convolution ---- */
/* nn.Conv2d(cin, cout, 7, 1, 3) [+ ReLU] [+ res1] on CB8, for the five shapes of SpyNet's BasicModule
 * (spynet_arch.py:17-22): (cin, cout) = (8, 32), (32, 64), (64, 32), (32, 16), (16, 2).  Every other pair is refused.
 *
 * sr_conv7x7_instance names the kernel instance a pair runs on, or -1 for a pair that is not served:
 *   0  conv7x7_f32_kernel<1, 4>: 32 couts x (16 rows x 32 columns) per workgroup — couts 32 and 16.  The 16 couts of (32, 16)
 *      run as 32 padded couts: twice the MFMA work of that layer, 50,176 extra FLOP per pixel, 10.5 % of a level's 479,808
 *   1  conv7x7_f32_kernel<2, 2>: 64 couts x (8 rows x 32 columns) — cout 64
 *   2  conv7x7_fewcout_f32_kernel: 4 couts x (16 rows x 32 columns) on v_mfma_f32_4x4x1_16b_f32 — cout 2 (padded to 4, not 32)
 * Instances 0 and 1 are implicit GEMMs on v_mfma_f32_32x32x2_f32.  Summation order of one output, from a zero accumulator, one
 * fused multiply-add per term: input channel block (8 channels) ascending, tap row ascending, tap column ascending, then
 * within the block the channel pairs (0, 4), (1, 5), (2, 6), (3, 7) (instance 2: channels 0..7); zero padding contributes
 * exact zeros.  Then + bias, max(., 0) when relu, + res1 — each one fp32 operation.  With K = 49 * cin terms,
 * |out - exact| <= (K + 2) * 2^-24 * (sum |w * x| + |bias| + |res1|) to first order.
 *
 * The packed image holds the weights in the instance's operand order followed by the bias (zeros for a NULL bias):
 * sr_conv7x7_packed_floats(cout, cin) floats in all, 0 for a pair that is not served.  Pad couts and pad channels are zero. */
int sr_conv7x7_instance(int cout, int cin);
size_t sr_conv7x7_packed_floats(int cout, int cin);
/* weight: OIHW [cout][cin][7][7]; bias: [cout] or NULL; packed: sr_conv7x7_packed_floats floats, 16-byte aligned.  Kernel id 151. */
int sr_conv7x7_pack_f32(const float* weight, const float* bias, int cout, int cin, float* packed, void* stream);

typedef struct sr_conv7x7_desc {
  const float* in;          /* CB8, cin / 8 blocks at h x w */
  long long in_img_stride;  /* floats between images */
  int cin, cout, n, h, w;
  const float* packed;      /* sr_conv7x7_pack_f32 of the same (cout, cin) */
  float* out;               /* CB8, ceil(cout / 8) blocks at h x w; pad channels of the last block are written 0 */
  long long out_img_stride;
  int relu;                 /* 0 / 1 */
  const float* res1;        /* NULL, or CB8 shaped like out: added after the activation */
  long long res1_img_stride;
} sr_conv7x7_desc;
/* out must not overlap in; res1 may be out.  Pointers 16-byte aligned, image strides multiples of 4 floats, every tensor
 * below 2^31 bytes per image.  Kernel ids 148 + instance. */
int sr_conv7x7_f32(const sr_conv7x7_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------- flow warping ---- */
#define SR_FLOW_NCHW 0
#define SR_FLOW_CB8 1
#define SR_FLOW_PAD_ZEROS 0
#define SR_FLOW_PAD_BORDER 1

/* F.grid_sample(x, grid(flow), 'bilinear', padding, align_corners=True) as flow_warp builds it.  x and out are [N][C][H][W]
 * (layout SR_FLOW_NCHW) or CB8 with ceil(C / 8) blocks (SR_FLOW_CB8; pad channels of x are never read, those of out are written
 * 0); flow is [N][H][W][2], (x, y) displacement in pixels.  Per output pixel (y, x), in fp32:
 *   ix = W > 1 ? (float)x + flow_x : 0;   iy = H > 1 ? (float)y + flow_y : 0      (one rounding each)
 *   border: ix = min(max(ix, 0), W - 1), likewise iy
 *   x0 = floor(ix), fx = ix - x0 (exact), likewise y0, fy
 * and, in float64 rounded once to fp32,
 *   out = (1 - fy) * ((1 - fx) * v(y0, x0) + fx * v(y0, x0 + 1)) + fy * ((1 - fx) * v(y0 + 1, x0) + fx * v(y0 + 1, x0 + 1))
 * where v of a position outside the image is 0 and is not read — so the far corner of a sample at exactly W - 1 or H - 1, whose
 * weight is 0, is not read either.  A coordinate that is not finite, or at or beyond -1 / W (H), gives 0 under zeros.
 * |out - exact(ix, iy)| <= 2^-24 * max |v|.  out must not overlap x or flow.  Kernel id 152. */
int sr_flow_warp_f32(const float* x, const float* flow, float* out, int N, int C, int H, int W, int layout, int padding,
                     void* stream);

/* The gradients of sr_flow_warp_f32 from g = dL/dout (laid out like out); dx or dflow may be NULL.
 *   dflow [N][H][W][2]: one thread per pixel, a float64 sum over the channels in channel order of
 *       g * ((1 - fy) * (v01 - v00) + fy * (v11 - v10))   and   g * ((1 - fx) * (v10 - v00) + fx * (v11 - v01)),
 *     rounded once: bit-reproducible.  Under border the component of an axis is 0 where its coordinate was clipped (strictly
 *     outside [0, size - 1]); it is 0 on an axis of size 1.
 *   dx (laid out like x): the CALLER zeroes it; the kernel adds g * corner weight (weight product in float64, rounded, times
 *     g in fp32) to each corner inside the image with atomicAdd(float*).  The last bits of an element that receives more than
 *     one contribution depend on the order in which the adds arrive: with d contributions |dx - exact| <= d * 2^-24 * sum
 *     |terms|, and two runs agree within that bound, not bit for bit.
 * Kernel ids 153 (dx) and 154 (dflow). */
int sr_flow_warp_bwd_f32(const float* x, const float* flow, const float* g, float* dx, float* dflow, int N, int C, int H,
                         int W, int layout, int padding, void* stream);

/* ---------------------------------------------------------------------------------------------------- SpyNet pieces ---- */
/* The 8-channel input block of one pyramid level (spynet_arch.py:64-77) in one launch:
 *   up        = 2 * F.interpolate(flow_prev, scale_factor=2, 'bilinear', align_corners=True)
 *   out       = cat(ref, flow_warp(supp, up, 'bilinear', 'border'), up)      3 + 3 + 2 channels = one CB8 block
 *   up_out    = up as a CB8 block (channels 0, 1; the rest 0): what the last conv of the level adds as res1
 * ref and supp are [N][3][H][W]; flow_prev is a CB8 block at (H / 2) x (W / 2) holding the flow in channels 0, 1 (H and W
 * even), or NULL for the coarsest level, whose incoming flow is zero: up = 0, warp = supp.  The source coordinate of the
 * upsampling, y * (Hp - 1) / (H - 1), and its blend are evaluated in float64 and rounded once; the warp is sr_flow_warp_f32's.
 * Kernel id 155. */
int sr_spynet_level_input_f32(const float* ref, const float* supp, const float* flow_prev, float* out, float* up_out, int N,
                              int H, int W, void* stream);

/* SpyNet.preprocess: out[n][c] = (x[n][c] - mean3[c]) / std3[c] on [N][3][H][W]; mean3 / std3 are host arrays.  Two fp32
 * operations, bit-identical to torch.  out may be x.  Kernel id 156. */
int sr_spynet_preprocess_f32(const float* x, float* out, int N, int H, int W, const float* mean3, const float* std3,
                             void* stream);

/* F.avg_pool2d(x, 2, 2) on `planes` planes of H x W (H, W even): out = ((a + b) + (c + d)) * 0.25f with a b / c d the window's
 * rows.  Kernel id 157. */
int sr_avgpool2x2_f32(const float* x, float* out, int planes, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_FLOW_H */
