/* libsr_hip.so — the recurrent video networks (basicsr/archs/basicvsr_arch.py), fp32 inference on gfx950: the input of one
 * propagation step in one launch, and one ConvResidualBlocks trunk call as one entry point.
 *
 * Declared apart from sr_hip.h and sr_hip_flow.h so that the existing ABI headers and their ledgers stay as they are; everything
 * here uses the types and status codes of sr_hip.h.  Launch-profiler id 159 (sr_kernel_name); 158 stays unnamed.  Bad arguments
 * return SR_EINVAL with a message in sr_last_error before anything is launched.  CB8 is the channel-blocked layout
 * [N][C/8][H][W][8] of sr_hip.h; a "window" is a run of channel blocks inside a wider CB8 tensor (pointer to its first block and
 * the image stride of the wider tensor).  Everything is bit-reproducible and independent of the batch. */
#ifndef SR_HIP_VSR_H
#define SR_HIP_VSR_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------- propagation step input ---- */
/* What one step of a propagation branch feeds its trunk (basicvsr_arch.py:62-68, :73-80), without intermediate tensors:
 *   frame_out  one CB8 block: channels 0-2 the frame, channels 3-7 zero                       (optional)
 *   warp_out   fb blocks: flow_warp(prev, flow, 'bilinear', 'zeros', align_corners=True), or exact zeros when prev is NULL
 * The warp is the flow-warp entry point's of sr_hip_flow.h (SR_FLOW_CB8, SR_FLOW_PAD_ZEROS) bit for bit: the same fp32 position, floor and exact fraction,
 * the float64 four-corner blend rounded once, no read of a corner outside the image (sr_hip_flow.h).  The flow is read as two
 * planes — what SpyNet returns — so no [N][H][W][2] copy is made.  Any H, W >= 1. */
typedef struct sr_vsr_prop_desc {
  const float* frame;              /* [3][H][W] per image (NCHW) */
  long long frame_img_stride;      /* floats between images: x[:, i] of a [b][n][3][h][w] clip is read in place */
  const float* prev;               /* CB8 window of fb blocks, or NULL: the first step of a branch */
  long long prev_img_stride;
  const float* flow;               /* [2][H][W] per image: plane 0 the x, plane 1 the y displacement in pixels; NULL iff prev is NULL */
  long long flow_img_stride;
  float* frame_out;                /* CB8 window of one block, or NULL */
  long long frame_out_img_stride;
  float* warp_out;                 /* CB8 window of fb blocks */
  long long warp_out_img_stride;
  int n, h, w, fb;                 /* fb = num_feat / 8 */
} sr_vsr_prop_desc;
/* The destinations must not overlap the sources or each other.  CB8 pointers 16-byte aligned, their image strides multiples of 4
 * floats; H * W < 2^28; n and fb + 1 at most 65535.  Kernel id 159. */
int sr_vsr_prop_input_f32(const sr_vsr_prop_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------- trunk driver ---- */
/* ConvResidualBlocks (basicvsr_arch.py:96-105) on a prepared CB8 input:
 *   conv 3x3 (3 + cin_segs * num_feat -> num_feat) + LeakyReLU(0.1), then num_block times x + conv2(relu(conv1(x)))
 * as 1 + 2 * num_block launches of the existing 3x3 kernels: the skip is res1 of conv2.  The first conv is segmented
 * (sr_conv3x3_pack_f32: first_seg = 3, seg = num_feat): the input holds the frame block, then cin_segs feature windows of
 * num_feat / 8 blocks, cin_pad = 8 + cin_segs * num_feat channels in all — 72 for BasicVSR, 136 for IconVSR's forward trunk.
 * Dispatch per conv is that of the RRDBNet inference forward: unless the Winograd switch is off (sr_dev_set_wino_f32(0)) a conv
 * with cout % 32 == 0 tries the Winograd F(2x2,3x3) kernel, which declines below 128 x 128 pixels unless a tile variant is forced;
 * a conv it declines runs on sr_conv3x3_f32's direct kernels.  num_feat must be a multiple of 8. */
typedef struct sr_vsr_trunk_cfg {
  int num_feat;   /* multiple of 8 */
  int num_block;  /* >= 0 */
  int cin_segs;   /* 1 or 2 */
} sr_vsr_trunk_cfg;

/* 2 * (1 + 2 * num_block): weight and bias of every conv in state_dict order (main.0, main.2.{i}.conv1, main.2.{i}.conv2);
 * SR_EINVAL for a bad config. */
int sr_vsr_trunk_num_params(const sr_vsr_trunk_cfg* cfg);
/* 1 where conv `index` (0 = the first conv, then conv1, conv2 of each block) has a Winograd image in the blob, 0 where not,
 * SR_EINVAL for a bad config or index. */
int sr_vsr_trunk_conv_wino(const sr_vsr_trunk_cfg* cfg, int index);
/* Bytes of the packed blob: the direct images of sr_conv3x3_pack_f32, behind them the Winograd images of the eligible convs, then
 * the table the pack launch reads.  0 for a bad config. */
size_t sr_vsr_trunk_packed_bytes(const sr_vsr_trunk_cfg* cfg);
/* params: sr_vsr_trunk_num_params device pointers (OIHW weights, biases); packed: sr_vsr_trunk_packed_bytes bytes, 256-byte
 * aligned.  One launch (pack_net_kernel). */
int sr_vsr_trunk_pack_f32(const sr_vsr_trunk_cfg* cfg, const float* const* params, float* packed, void* stream);
/* Bytes of the three activation buffers a call on n images of h x w rotates through (input, ReLU output, block output: a conv never
 * writes the tensor it reads as res1).  Three, not the two of a plain ping-pong: with two, conv2 would have to write the buffer it
 * reads as res1, and sr_conv3x3_f32 and the Winograd kernel do not promise that out may alias res1.  0 for a bad config or shape. */
size_t sr_vsr_trunk_workspace_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w);
/* in: CB8 window of 1 + cin_segs * num_feat / 8 blocks; out: CB8 window of num_feat / 8 blocks, not overlapping in or the
 * workspace.  Allocates, copies and synchronises nothing: 1 + 2 * num_block launches on `stream`. */
int sr_vsr_trunk_f32(const sr_vsr_trunk_cfg* cfg, const float* packed, const float* in, long long in_img_stride, float* out,
                     long long out_img_stride, int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_VSR_H */
