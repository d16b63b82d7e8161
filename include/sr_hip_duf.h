/* libsr_hip.so — the pieces of DUF (basicsr/archs/duf_arch.py) that no other header has, fp32 on gfx950: the 3D convolutions
 * over (time, height, width) with kernel (1, 3, 3) and (3, 3, 3), the 1x1x1 convolution of the dense blocks, both with an
 * optional eval-mode BatchNorm3d -> ReLU on their input, and the tail of the network (softmax over the 25 taps, the 5x5 dynamic
 * filter on the centre frame, the residual and the pixel shuffle) in one launch.  The four 1x1x1 head convolutions run on
 * sr_convd_f32 (ksize 1) of the RIDNet header.
 *
 * Declared apart from sr_hip.h so that the existing ABI headers and their ledgers stay as they are; everything here uses the
 * types and status codes of sr_hip.h.  Launch-profiler ids 194-197 (sr_kernel_name); 193 stays unnamed.
 * Bad arguments return SR_EINVAL with a message in sr_last_error before anything is launched.  Nothing allocates or
 * synchronises.  Every kernel is bit-reproducible and independent of the batch (clip i of a batch gets what a batch of that
 * clip alone gets) and uses no atomics.
 *
 * Layout.  A clip's activations are frame-major CB8, [b][T][C/8][h][w][8]: frame t of clip i is a CB8 image of sr_hip.h at
 * base + i * clip_stride + t * frame_stride (floats).  A dense concatenation is one such buffer allocated at its final channel
 * count: a convolution reads the channel prefix (the first ceil(cin / 8) blocks of every frame) and writes its couts at a
 * channel-block offset of the same frames, so torch.cat costs no copy; cat(x[:, :, 1:-1], conv(x)) of the temporal-reduce
 * blocks is the same buffer with the destination one frame further on. */
#ifndef SR_HIP_DUF_H
#define SR_HIP_DUF_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One descriptor for both convolutions. */
typedef struct sr_duf_conv_desc {
  const float* in;             /* frame-major CB8, ceil(cin / 8) blocks of every frame are read */
  long long in_frame_stride;   /* floats between frames of a clip */
  long long in_clip_stride;    /* floats between clips */
  int cin, cout;
  int kt, pad_t;               /* temporal taps and temporal zero padding: (1, 0), (3, 0) or (3, 1); the 1x1x1 conv takes (1, 0) */
  int b, t, h, w;              /* clips, input frames per clip, frame size */
  const float* packed;         /* the pack entry point's image of the same (cout, cin, kt) */
  const float* scale;          /* input prologue: [cin] each, both or neither */
  const float* shift;
  float* out;                  /* frame-major CB8; t_out = t - 2 * (1 - pad_t) frames for kt = 3, t for kt = 1 */
  long long out_frame_stride;
  long long out_clip_stride;
  int out_cb0;                 /* channel block of every destination frame that receives cout 0 */
  int relu;                    /* 0 / 1 */
} sr_duf_conv_desc;

/* ------------------------------------------------------------------------------------------------ 3D convolution ---- */
/* nn.Conv3d(cin, cout, (kt, 3, 3), 1, (pad_t, 1, 1)) [+ ReLU], kt in {1, 3}, pad_t in {0, 1} (0 when kt = 1).
 * cin: a multiple of 8 up to 448, or 3 stored as one block (conv3d1: channels 3-7 of the block are replaced by zero before
 * the multiply, whatever they hold).  cout in {16, 32, 64, 256}.  Everything else is refused.
 *
 * Input prologue (scale and shift given): the operand is max(x * scale[c] + shift[c], 0) — one multiply, one add, one max, in
 * that order, each rounded to fp32 — applied as the tile is staged.  This is eval-mode BatchNorm3d -> ReLU in front of the
 * convolution.  Zero padding, spatial and temporal, is applied AFTER the prologue: a padded position contributes exact zero,
 * not max(shift, 0).  Frames outside the clip contribute zero; the last frame of clip i never reads the first of clip i + 1.
 *
 * duf_conv3d_f32_kernel: an implicit GEMM D[cout][pixel] += W[cout][k] * X[k][pixel] on v_mfma_f32_16x16x4_f32 for EVERY cout,
 * 16 included: a 32x32x2 tile would waste half its columns at cout = 16, 16x16x4 wastes none, and both shapes have the same
 * peak rate (64 FLOP/clk/SIMD).  A workgroup of 4 waves computes 8 rows x 32 columns x min(cout, 64) couts of one output
 * frame (cout = 256: four cout groups in grid.y); a wave owns 2 rows = four 16-pixel groups and 1 / 2 / 4 tiles of 16 couts:
 * 16 / 32 / 64 accumulator registers.  K is walked in chunks of (one 8-channel block, one frame tap): the halo'd tile
 * [10][34][8] (10.6 KiB) and the 9 taps of weights [9][couts][8] (4.5 / 9 / 18 KiB) go global -> registers -> LDS (the
 * prologue is applied between the two), double buffered with one barrier per chunk: 30.3 / 39.3 / 57.3 KiB and 96 / 116 / 158
 * VGPRs, so at least two workgroups share a CU (two waves per SIMD) in every instance.
 * Summation order of one output, from a zero accumulator, one fused multiply-add per term: input channel block ascending,
 * frame tap ascending (frames outside the clip are skipped), tap row ascending, tap column ascending, then within the block
 * the channels (0, 2, 4, 6) and (1, 3, 5, 7); zero padding and pad channels contribute exact zeros.  Then + bias, max(., 0)
 * when relu — each one fp32 operation.  With K = 9 * kt * cin_pad terms (cin_pad = cin rounded up to 8),
 *   |out - exact| <= (K + 2) * 2^-24 * (sum |w * x| + |bias|)   to first order, x the operand after the prologue.
 *
 * sr_duf_conv3d_packed_floats(cout, cin, kt): floats of the packed image (weights in operand order
 * [cout group][cin block][frame tap][tap row][tap column][couts][8 channels], then the biases, zeros for NULL); 0 for a
 * triple that is not served. */
size_t sr_duf_conv3d_packed_floats(int cout, int cin, int kt);
/* weight: OIDHW [cout][cin][kt][3][3]; bias: [cout] or NULL; packed: 16-byte aligned.  Kernel id 195. */
int sr_duf_conv3d_pack_f32(const float* weight, const float* bias, int cout, int cin, int kt, float* packed, void* stream);
/* out must not overlap what is read of in (another channel range of the same buffer is fine).  Pointers 16-byte aligned,
 * strides multiples of 4 floats, a frame below 2^31 bytes.  Kernel id 194. */
int sr_duf_conv3d_f32(const sr_duf_conv_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------- 1x1x1 convolution ---- */
/* nn.Conv3d(c, c, 1) [+ ReLU] with the same optional input prologue: the first convolution of every dense block, on the
 * channel-prefix read.  cin == cout == c, a multiple of 8 up to 432; kt = 1, pad_t = 0.  The BatchNorm3d behind the
 * convolution is the caller's to fold into weight and bias.
 * duf_pw_f32_kernel: the kernel above with one tap and no halo, 64 couts per cout group (the image is zero padded to a
 * multiple of 64 couts; only c / 8 blocks are written): [8][32][8] (8 KiB) + [64][8] (2 KiB) per chunk of 8 channels, double
 * buffered.  Summation order: channel block ascending, within it (0, 2, 4, 6) then (1, 3, 5, 7); bound as above with K = c.
 * Image: [cout group][cin block][64 couts][8 channels], then the biases. */
size_t sr_duf_pw_packed_floats(int c);
/* weight: [c][c] (OIDHW with 1x1x1 taps); bias: [c] or NULL.  Kernel id 195. */
int sr_duf_pw_pack_f32(const float* weight, const float* bias, int c, float* packed, void* stream);
/* Kernel id 196. */
int sr_duf_pw_f32(const sr_duf_conv_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------ dynamic filter ---- */
/* The tail of DUF.forward (duf_arch.py:276-281) in one launch, s in {2, 3, 4}:
 *   f   = softmax ? softmax over the 25 taps of logits.view(n, 25, s*s, h, w) : that view itself
 *   out[n][c * s*s + sub][y][x] = sum_tap f[n][tap][sub][y][x] * centre[n][c][y + tap / 5 - 2][x + tap % 5 - 2]   (zero padding)
 *                                 + (res ? res[n][c * s*s + sub][y][x] : 0)
 *   shuffle ? pixel_shuffle(out, s) as NCHW [n][3][s*h][s*w] : out as NCHW [n][3*s*s][h][w]
 * logits: CB8, 25*s*s channels, channel = tap * s*s + sub; res: CB8, 3*s*s channels, or NULL; the CB8 pad channels are never
 * read.  centre: [3][h][w] of image n at centre + n * centre_img_stride, read in place from the input clip.  Any h, w >= 1.
 * One thread per (pixel, sub).  Softmax: m = max over the taps, e = expf(l - m), sum of e in tap order, e / sum — so +-80
 * logits do not overflow.  Then per colour, from zero, tap ascending: one multiply and one add per tap; then + res.
 * The error against exact arithmetic is a few ulp of the 25 weights (expf) plus 27 * 2^-24 * sum |f * x|.
 * Strides in floats; CB8 tensors 16-byte aligned.  Kernel id 197. */
int sr_duf_filter_f32(const float* logits, long long logits_img_stride, const float* res, long long res_img_stride,
                      const float* centre, long long centre_img_stride, float* out, int n, int s, int h, int w, int softmax,
                      int shuffle, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_DUF_H */
