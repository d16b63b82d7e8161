/* libsr_hip.so — the backward of SpyNet's building blocks (sr_hip_flow.h), fp32 on gfx950: the data gradient and the weight
 * gradient of the 7x7 convolution, the adjoint of a pyramid level's input block and the adjoint of the bilinear resize.
 *
 * Declared apart from sr_hip_flow.h so that the forward header and its ledger stay as they are; everything here uses the types and
 * status codes of sr_hip.h and the CB8 layout [N][C/8][H][W][8].  Launch-profiler ids 169-176 (sr_kernel_name); 168 stays unnamed.
 * Bad arguments return SR_EINVAL with a message in sr_last_error before anything is launched.  No kernel here uses an atomic: every
 * result is bit-reproducible, and image n of a batch gets from the data gradient and the adjoints what a batch of that image alone
 * gets.  (cin, cout) below is always the FORWARD convolution's pair: (8, 32), (32, 64), (64, 32), (32, 16), (16, 2). */
#ifndef SR_HIP_FLOW_BWD_H
#define SR_HIP_FLOW_BWD_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --------------------------------------------------------------------------------------------------- 7x7 data gradient ---- */
/* dx = (dy * flipped, transposed W) . (mask > 0):  dx[ci][y][x] = sum over co, ty, tx of dy[co][y - ty + 3][x - tx + 3] *
 * W[co][ci][ty][tx], a 7x7 convolution of dy (cout channels) into dx (cin channels) with the weight image of
 * sr_conv7x7_dgrad_pack_f32.  It runs on the forward's implicit-GEMM body (v_mfma_f32_32x32x2_f32, LDS-DMA staging by tap rows,
 * double buffering, two workgroups per CU); sr_conv7x7_dgrad_instance names the instance, -1 for a pair that is not served:
 *   0  conv7x7_dgrad_f32_kernel<1, 4>: 32 dx channels x (16 rows x 32 columns) per workgroup — dx channels 8, 16 and 32
 *   1  conv7x7_dgrad_f32_kernel<2, 2>: 64 dx channels x (8 rows x 32 columns) — dx channels 64, the pair (64, 32)
 * (32, 64) [dy 64 -> dx 32] and (64, 32) [dy 32 -> dx 64] are the forward's own shapes and carry no padding.  The other three
 * run on instance 0, the 32-wide tile, because the dx channel counts 8 and 16 have no smaller MFMA tile in the body and these
 * layers are the cheap ones; MFMA work per pixel (2 * 49 * K * M FLOP), real -> run:
 *   (8, 32)   dy 32 -> dx 8:    25,088 -> 100,352   the 8 dx channels run as 32
 *   (32, 16)  dy 16 -> dx 32:   50,176 ->  50,176   K = 16 is two whole blocks, M = 32: no padding
 *   (16, 2)   dy 2 -> dx 16:     3,136 ->  25,088   K: the 2 dy channels are one 8-channel block; M: 16 run as 32
 * — 97,216 extra FLOP per pixel, 20.3 % of a level's 479,808 data-gradient FLOP.
 * Summation order of one output, from a zero accumulator, one fused multiply-add per term: dy channel block (8 channels) ascending,
 * tap row of the flipped kernel ascending, tap column ascending, then within the block the channel pairs (0, 4), (1, 5), (2, 6),
 * (3, 7); zero padding contributes exact zeros.  Then the mask: an element whose mask element is not > 0 becomes 0.  With
 * K = 49 * 8 * ceil(cout / 8) terms, |dx - exact| <= K * 2^-24 * sum |w * dy| to first order.
 *
 * The packed image holds W flipped and transposed in the instance's operand order, then one zero per padded dx channel (the body's
 * bias slot): sr_conv7x7_dgrad_packed_floats(cout, cin) floats, 0 for a pair that is not served. */
int sr_conv7x7_dgrad_instance(int cout, int cin);
size_t sr_conv7x7_dgrad_packed_floats(int cout, int cin);
/* weight: OIHW [cout][cin][7][7]; packed: sr_conv7x7_dgrad_packed_floats floats, 16-byte aligned.  Kernel id 171. */
int sr_conv7x7_dgrad_pack_f32(const float* weight, int cout, int cin, float* packed, void* stream);

typedef struct sr_conv7x7_dgrad_desc {
  const float* dy;           /* CB8, ceil(cout / 8) blocks at h x w; pad channels of the last block must be finite (they meet zero weights) */
  long long dy_img_stride;   /* floats between images */
  int cin, cout, n, h, w;    /* the forward conv's pair */
  const float* packed;       /* sr_conv7x7_dgrad_pack_f32 of the same (cout, cin) */
  float* dx;                 /* CB8, cin / 8 blocks at h x w */
  long long dx_img_stride;
  const float* mask;         /* NULL, or CB8 shaped like dx: the post-ReLU activation that fed the forward conv */
  long long mask_img_stride;
} sr_conv7x7_dgrad_desc;
/* dx must not overlap dy; mask may be dx.  Pointers 16-byte aligned, image strides multiples of 4 floats, every tensor below 2^31
 * bytes per image.  Kernel ids 169 + instance. */
int sr_conv7x7_dgrad_f32(const sr_conv7x7_dgrad_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------- 7x7 weight gradient ---- */
/* dweight[co][ci][ty][tx] (+)= scale * sum over n, y, x of dy[co][y][x] * x[ci][y + ty - 3][x + tx - 3]   (x zero outside the image)
 * dbias[co]               (+)= scale * sum over n, y, x of dy[co][y][x]                                  (dbias may be NULL)
 * on v_mfma_f32_32x32x2_f32 with the pixels as the GEMM's K: D[32 couts][32 cins] += dy[32 couts][2 pixels] * x[2 pixels][32 cins].
 * One workgroup owns (a 32 x 32 channel tile, ONE TAP ROW ty, a strip of 32 columns x RW rows of one image): 7 taps x 16 = 112
 * accumulator registers per wave.  Wave w takes the strip's rows 4 t + w; per dy row it stages that row (32 pixels x 32 couts) and
 * the one x row y + ty - 3 (38 pixels x 32 cins) by LDS-DMA, double buffered, reads them into registers once (16 + 37 ds_read_b32
 * per lane) and issues 16 x 7 MFMAs.  Because a workgroup has one tap row, a dy row meets exactly one x row and no row ring is
 * needed; the price is that x is read once per tap row (7 times in all, from L2).  The four waves' tiles are added through LDS as
 * (w0 + w2) + (w1 + w3) and written to the caller's slab; conv7x7_wgrad_reduce_kernel adds the strips in ascending strip order
 * (image, then row chunk, then column tile), multiplies by scale and stores or adds (accumulate = 1: into a FlatAdam arena).
 *
 * The plan, also what sr_conv7x7_wgrad_slab_bytes sizes: CT = ceil(cout / 32), IT = ceil(cin / 32), TX = ceil(w / 32),
 *   chunks = min(max(ceil(1024 / (n * TX * CT * IT * 7)), 1), ceil(h / 4));  RW = 4 * ceil(ceil(h / chunks) / 4);  chunks = ceil(h / RW)
 *   NP = n * chunks * TX strips;   slab = 4 * NP * (CT * IT * 49 * 1024 + CT * 64) bytes.
 * Channel padding (the tile is always 32 x 32; absent channel blocks are the zero fill of the buffer loads), MFMA work real -> run:
 *   (8, 32): 1 / 4 useful (8 cins as 32)      (32, 64), (64, 32): all useful      (32, 16): 1 / 2 (16 couts as 32)
 *   (16, 2): 1 / 32 (2 couts as 32, 16 cins as 32): 100,352 FLOP per pixel run for 3,136
 * — the five layers run 702,464 FLOP per pixel for 479,808 real ones; a smaller tile for (16, 2) and (8, 32) would save 25 %.
 * Summation order of one element: within a wave pixels left to right, rows 4 t + w ascending, one fused multiply-add per pixel into
 * a zero accumulator; then the adds above.  With T = 32 * RW / 4 terms per wave and A = 2 + NP reduction adds,
 *   |dweight - exact| <= (T + A) * 2^-24 * sum |dy * x| * |scale| + 2 * 2^-24 * |exact|   to first order
 * (the last term: the multiplication by scale and the accumulating add); dbias likewise with sum |dy|. */
size_t sr_conv7x7_wgrad_slab_bytes(int n, int h, int w, int cout, int cin);

typedef struct sr_conv7x7_wgrad_desc {
  const float* x;            /* CB8, cin / 8 blocks at h x w: the forward conv's input */
  long long x_img_stride;
  const float* dy;           /* CB8, ceil(cout / 8) blocks at h x w */
  long long dy_img_stride;
  int cin, cout, n, h, w;
  float scale;
  float* dweight;            /* OIHW [cout][cin][7][7] */
  float* dbias;              /* [cout] or NULL */
  int accumulate;            /* 0: store, 1: add to what dweight / dbias hold */
  void* slab;                /* sr_conv7x7_wgrad_slab_bytes bytes, 16-byte aligned */
  size_t slab_bytes;
} sr_conv7x7_wgrad_desc;
/* Pointers 16-byte aligned (dweight, dbias: 4), image strides multiples of 4 floats, every tensor below 2^31 bytes per image.
 * Kernel ids 172 (tiles) and 173 (reduction). */
int sr_conv7x7_wgrad_f32(const sr_conv7x7_wgrad_desc* d, void* stream);

/* ------------------------------------------------------------------------------------- adjoint of a level's input block ---- */
/* The backward of the level-input entry point of sr_hip_flow.h with respect to flow_prev, in two launches:
 *   d_up[n][y][x]   = (g_res[0:2] + g_in[6:8]) + dflow        two fp32 additions per component
 *   g_prev          = 2 * U^T d_up                            as a CB8 block at (H / 2) x (W / 2): channels 0, 1; the rest 0
 * supp is [N][3][H][W]; up (the saved up_out), g_in (the gradient of the level's 8-channel input block) and g_res (the gradient of
 * the level's output flow, which reaches up through res1) are one-block CB8 tensors at H x W.  dflow is what the flow-warp
 * backward of sr_hip_flow.h writes on (supp, up[0:2], g_in[3:6], border): a float64 sum over the three channels, rounded once,
 * 0 on an axis whose coordinate was clipped.  U is the x2 align_corners=True upsampling of that entry point, coordinates in float64 as
 * there.  U^T is a gather: the thread of coarse pixel (yp, xp) visits the fine rows, then columns, in ascending order, and adds
 * wy * wx * d_up in float64 for each fine pixel that read (yp, xp) — wy, wx the float64 blend weights of the forward — and rounds
 * 2 * sum once: |g_prev - exact(d_up)| <= 2^-24 * |exact|.  d_up is the caller's [N][H][W][2] buffer (8-byte aligned).  H and W
 * even.  Gradients with respect to ref and supp are not computed.  Kernel ids 174 (d_up) and 175 (U^T). */
int sr_spynet_level_input_bwd_f32(const float* supp, const float* up, const float* g_in, const float* g_res, float* d_up,
                                  float* g_prev, int N, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------ adjoint of the final resize ---- */
/* dx = R^T dy for R = the bilinear resize of sr_hip_degrade.h from Hs x Ws to Hd x Wd without size arrays, on `planes` planes:
 * dy is [planes][Hd][Wd], dx [planes][Hs][Ws].  A gather: the thread of source pixel (ys, xs) visits the destination rows, then
 * columns, in ascending order, evaluates the forward's own float32 coordinate rule for each and adds wy * wx * dy in float64 where
 * that pixel read (ys, xs); rounded once: |dx - exact| <= 2^-24 * |exact|.  planes at most 65535.  Kernel id 176. */
int sr_resize_bilinear_adjoint_f32(const float* dy, float* dx, int planes, int Hs, int Ws, int Hd, int Wd, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_FLOW_BWD_H */
