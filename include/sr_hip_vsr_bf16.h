/* libsr_hip.so — the recurrent video networks (basicsr/archs/basicvsr_arch.py), bf16 inference on gfx950: the input of one
 * propagation step in one launch, and one ConvResidualBlocks trunk call as one entry point, both on CB16 activations.
 *
 * The bf16 twin of the fp32 header of the recurrent video networks, declared apart from it so that the existing ABI headers and
 * their ledgers stay as they are; everything here uses the types and status codes of sr_hip.h and the trunk configuration struct
 * of the fp32 header.  Launch-profiler id 167 (sr_kernel_name); 166 stays unnamed.  Bad arguments return SR_EINVAL with a message
 * in sr_last_error before anything is launched.  CB16 is the channel-blocked bf16 layout [N][C/16][H][W][16] of sr_hip.h (32-byte
 * pixels); a "window" is a run of channel blocks inside a wider CB16 tensor (pointer to its first block and the image stride of
 * the wider tensor, in bf16 ELEMENTS).  Everything is bit-reproducible and independent of the batch. */
#ifndef SR_HIP_VSR_BF16_H
#define SR_HIP_VSR_BF16_H

#include "sr_hip.h"
#include "sr_hip_vsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------- propagation step input ---- */
/* What one step of a propagation branch feeds its trunk (basicvsr_arch.py:62-68, :73-80), without intermediate tensors:
 *   frame_out  one CB16 block: channels 0-2 bf16(frame), round to nearest even, channels 3-15 zero          (optional)
 *   warp_out   fb blocks: the previous feature warped by the flow (bilinear, zeros padding, align_corners=True), or exact
 *              zeros when prev is NULL
 * The warp's arithmetic is that of the fp32 step-input kernel on the widened corners: the four bf16 corners widened to fp32
 * (exact), the same fp32 position with one rounding, floor and exact fraction, the same in-image corner rule (no read of a
 * corner outside the image), the float64 four-corner blend rounded once to fp32, and that value rounded to bf16, nearest even.
 * So warp_out is bit for bit bf16(the fp32 zeros-padding warp of the widened prev).  The flow stays fp32: two planes, what SpyNet
 * returns (a displacement of 16 px stored in bf16 would sit on a 1/8 px grid).  Any H, W >= 1. */
typedef struct sr_rvsr_prop_desc {
  const float* frame;              /* fp32 [3][H][W] per image (NCHW) */
  long long frame_img_stride;      /* floats between images: x[:, i] of a [b][n][3][h][w] clip is read in place */
  const void* prev;                /* bf16 CB16 window of fb blocks, or NULL: the first step of a branch */
  long long prev_img_stride;       /* bf16 elements */
  const float* flow;               /* fp32 [2][H][W] per image: plane 0 the x, plane 1 the y displacement in pixels; NULL iff prev is NULL */
  long long flow_img_stride;       /* floats */
  void* frame_out;                 /* bf16 CB16 window of one block, or NULL */
  long long frame_out_img_stride;  /* bf16 elements */
  void* warp_out;                  /* bf16 CB16 window of fb blocks */
  long long warp_out_img_stride;   /* bf16 elements */
  int n, h, w, fb;                 /* fb = num_feat / 16 */
} sr_rvsr_prop_desc;
/* The destinations must not overlap the sources or each other.  CB16 pointers 16-byte aligned, their image strides multiples of 8
 * elements; frame / flow 4-byte aligned; H * W < 2^28; n and fb + 1 at most 65535.  Kernel id 167. */
int sr_rvsr_prop_input_bf16(const sr_rvsr_prop_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------- trunk driver ---- */
/* ConvResidualBlocks (basicvsr_arch.py:96-105) on a prepared CB16 input:
 *   conv 3x3 (3 + cin_segs * num_feat -> num_feat) + LeakyReLU(0.1), then num_block times x + conv2(relu(conv1(x)))
 * as 1 + 2 * num_block plain launches of sr_conv3x3_bf16 (never the persistent conv chain): the skip is res1 of conv2, beta1 = 1,
 * one rounding per conv output.  The first conv is segmented (sr_conv3x3_pack_bf16: first_seg = 3, seg = num_feat): the input
 * holds the frame block, then cin_segs feature windows of num_feat / 16 blocks, cin_pad = 16 + cin_segs * num_feat channels in
 * all — 80 for BasicVSR, 144 for IconVSR's forward trunk.  The configuration is the fp32 header's struct, and the number of
 * parameters is that header's query; num_feat must be a multiple of 16 here. */

/* Bytes of the packed blob: per conv the bf16 image of sr_conv3x3_pack_bf16 and the fp32 packed bias, each padded to 256 bytes,
 * then the table the pack launch reads.  0 for a bad config. */
size_t sr_rvsr_trunk_packed_bytes_bf16(const sr_vsr_trunk_cfg* cfg);
/* params: 2 * (1 + 2 * num_block) device pointers to the fp32 masters in state_dict order (OIHW weights, biases); packed:
 * sr_rvsr_trunk_packed_bytes_bf16 bytes, 256-byte aligned.  One memset, one table copy, one launch (the pack table). */
int sr_rvsr_trunk_pack_bf16(const sr_vsr_trunk_cfg* cfg, const float* const* params, void* packed, void* stream);
/* Bytes of the three activation buffers a call on n images of h x w rotates through (block input, ReLU output, block output): three
 * because a conv must not write the tensor it reads as res1.  0 for a bad config or shape. */
size_t sr_rvsr_trunk_workspace_bytes_bf16(const sr_vsr_trunk_cfg* cfg, int n, int h, int w);
/* in: CB16 window of 1 + cin_segs * num_feat / 16 blocks; out: CB16 window of num_feat / 16 blocks, not overlapping in or the
 * workspace; image strides in bf16 elements, multiples of 8.  SR_ENOSPACE for a short workspace (none is needed with num_block = 0).
 * Allocates, copies and synchronises nothing: 1 + 2 * num_block launches on `stream`. */
int sr_rvsr_trunk_bf16(const sr_vsr_trunk_cfg* cfg, const void* packed, const void* in, long long in_img_stride, void* out,
                       long long out_img_stride, int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_VSR_BF16_H */
