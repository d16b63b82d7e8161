/* libsr_hip.so — the recurrent backward of BasicVSR (sr_hip_vsr.h is the forward), fp32 on gfx950: the adjoint of the input of one
 * propagation step in one launch, the trunk call that keeps what its backward reads, and that backward as one call.
 *
 * Declared apart from sr_hip_vsr.h so that the forward header and its ledger stay as they are; everything here uses the types and
 * status codes of sr_hip.h, the trunk config of sr_hip_vsr.h and the CB8 layout [N][C/8][H][W][8]; a "window" is a run of channel
 * blocks inside a wider CB8 tensor.  Launch-profiler id 178 (sr_kernel_name); 177 stays unnamed.  Bad arguments return SR_EINVAL
 * with a message in sr_last_error before anything is launched.  The scatter into dprev of the step-input adjoint is the ONE step of
 * the whole backward that uses an atomic and is not bit-reproducible; everything else here is, and is independent of the batch. */
#ifndef SR_HIP_VSR_BWD_H
#define SR_HIP_VSR_BWD_H

#include "sr_hip.h"
#include "sr_hip_vsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------------------------- adjoint of the propagation step input ---- */
/* The backward of the forward header's step input with respect to prev and flow, from g = dL/dwarp_out, in ONE launch and in
 * place: the flow is read as the two planes the forward read, prev and dprev are windows, dprev is added into (it already holds
 * the head's gradient of that frame's feature) and dflow is stored as two planes, straight into a [b][n - 1][2][h][w] gradient.
 * The generic warp backward of sr_hip_flow.h would need four more tensors per step for the same (a [N][H][W][2] copy of the flow,
 * prev copied out of its window, a zeroed dx that is then added, dflow copied back to planes).
 *
 * The sample position, the cell and the fractions fx, fy are the forward's bit for bit (zeros padding: the fp32 position
 * x + flow, floor, exact fraction).  A corner outside the image is neither read nor written.  A pixel whose position is not
 * finite or lies outside (-1, W) x (-1, H) gets dflow = 0 and adds nothing.  With v00, v01, v10, v11 the four corners of prev
 * (0 outside the image) and c running over the 8 * fb channels:
 *   dflow x = sum_c g[c] * ((1 - fy) * (v01 - v00) + fy * (v11 - v10)),   dflow y = sum_c g[c] * ((1 - fx) * (v10 - v00) + fx * (v11 - v01))
 *     a gather, every operation in float64.  Order: a lane owns (pixel, channel e of a block) and adds its term of block 0, 1, ...
 *     fb - 1 to a zero accumulator; the eight lanes of a pixel are then added as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)),
 *     and the sum is rounded to fp32 once.  Bit-reproducible and independent of the batch; 0 on an axis of size 1.
 *     |dflow - exact| <= 2^-24 |exact| + 2^-50 * sum |terms|, a term being g[c] * (blend weight derivative) * one corner.
 *   dprev[corner q] += g[c] * w_q   with w_q = (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx: the weight product and its
 *     product with g in float64, rounded to fp32 ONCE, added with atomicAdd(float*); a zero w_q adds nothing.  (The generic warp
 *     backward rounds the weight and then the product: two roundings a term, 2 + d in all, which the bound below does not cover
 *     for d = 1; rounding once makes it 1 + d.)  Lanes run over (pixel, channel in the
 *     block) with the channel fastest: a wave instruction adds eight 32-byte runs, which are contiguous where the flow is locally
 *     constant.  The kernel never zeroes dprev.  The last bits of an element depend on the order in which the adds arrive: with d
 *     contributions |dprev - (before + exact)| <= (d + 1) * 2^-24 * (|before| + sum |terms|), and two runs agree within that
 *     bound, not bit for bit. */
typedef struct sr_vsr_prop_bwd_desc {
  const float* g;                  /* CB8 window of fb blocks: the gradient of warp_out */
  long long g_img_stride;
  const float* prev;               /* CB8 window of fb blocks: the feature that was warped */
  long long prev_img_stride;
  const float* flow;               /* [2][H][W] per image, as the forward read it */
  long long flow_img_stride;
  float* dprev;                    /* CB8 window of fb blocks, ADDED into; or NULL */
  long long dprev_img_stride;
  float* dflow;                    /* [2][H][W] per image, stored; or NULL */
  long long dflow_img_stride;
  int n, h, w, fb;
} sr_vsr_prop_bwd_desc;
/* dprev and dflow must not overlap the sources or each other; one of them at least is given.  CB8 pointers 16-byte aligned,
 * their image strides multiples of 4 floats; flow and dflow 4-byte aligned; any H, W >= 1 with H * W < 2^28; n and fb + 1 at most
 * 65535.  Kernel id 178. */
int sr_vsr_prop_input_bwd_f32(const sr_vsr_prop_bwd_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------- the trunk, activations kept ---- */
/* The forward header's trunk call with the same config, the same packed blob and the same per-conv dispatch — it IS that driver,
 * told to number its activations instead of rotating three buffers, so `out` is bit-equal under every setting of the Winograd
 * switch.  The stack is 2 * num_block buffers of A = roundup256(4 * n * num_feat * h * w) bytes, each a contiguous CB8 tensor:
 *   buffer 0          the post-LeakyReLU output of the first conv (the input of block 0)
 *   buffer 1 + 2 b    the post-ReLU output of conv1 of block b
 *   buffer 2 + 2 b    the output of block b, for b < num_block - 1
 * and the output of the last block goes to `out`.  With num_block = 0 the stack is empty (NULL passes) and `out` is the first
 * conv's output.  sr_vsr_trunk_keep_bytes is 2 * num_block * A, 0 for a bad config or shape.  1 + 2 * num_block launches; nothing
 * allocates or synchronises. */
size_t sr_vsr_trunk_keep_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w);
int sr_vsr_trunk_keep_f32(const sr_vsr_trunk_cfg* cfg, const float* packed, const float* in, long long in_img_stride, float* out,
                          long long out_img_stride, int n, int h, int w, void* stack, size_t stack_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------- the trunk's backward ---- */
/* The data-gradient images (sr_conv3x3_pack_f32's mode 1) of every conv of a trunk in one blob, in state_dict order, each offset a
 * multiple of 256 bytes, the pack table behind them; the first conv's image is segmented like its forward image (first_seg = 3,
 * seg = num_feat), so its data gradient is laid out like the trunk's input: the frame block, then the feature windows.  params:
 * the forward pack's array (biases are not read).  One launch.  sr_vsr_trunk_packed_dgrad_bytes: 0 for a bad config. */
size_t sr_vsr_trunk_packed_dgrad_bytes(const sr_vsr_trunk_cfg* cfg);
int sr_vsr_trunk_pack_dgrad_f32(const sr_vsr_trunk_cfg* cfg, const float* const* params, float* packed, void* stream);

/* 3 * A + roundup256(sr_conv3x3_wgrad_slab_bytes(n, h, w)): two gradient buffers that alternate (a conv never writes the tensor it
 * reads as res1), one for the gradient behind a ReLU, and the weight-gradient slab.  0 for a bad config or shape. */
size_t sr_vsr_trunk_bwd_workspace_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w);

typedef struct sr_vsr_trunk_bwd_desc {
  const float* packed_dgrad;       /* sr_vsr_trunk_pack_dgrad_f32 of the forward's parameters, 256-byte aligned */
  const float* in;                 /* the forward's input window: 1 + cin_segs * num_feat / 8 blocks */
  long long in_img_stride;
  const float* out;                /* the forward's output window; read only when num_block == 0 (it is the LeakyReLU mask) */
  long long out_img_stride;
  const void* stack;               /* what the keeping forward wrote */
  size_t stack_bytes;
  const float* dout;               /* CB8 window of num_feat / 8 blocks: dL/dout */
  long long dout_img_stride;
  float* din;                      /* CB8 window laid out like `in`: block 0 gets the frame block's gradient, the blocks behind
                                      it dL/d(feature windows); NULL: the first conv's data gradient is not run */
  long long din_img_stride;
  float* const* dparams;           /* 2 * (1 + 2 * num_block) targets in state_dict order (dweight OIHW, dbias); NULL: skip */
  int accumulate;                  /* 0: store, 1: add to what the targets hold */
  int n, h, w;
  void* workspace;                 /* sr_vsr_trunk_bwd_workspace_bytes bytes, 256-byte aligned */
  size_t workspace_bytes;
} sr_vsr_trunk_bwd_desc;
/* The adjoint of the keeping forward as one C call over the existing kernels, from the last conv to the first.  Per conv: the weight
 * gradient (sr_conv3x3_wgrad_f32; the first conv with first_seg = 3, seg = num_feat) when a target of the conv is given — a conv
 * whose two targets are NULL launches nothing, a bias target without its weight target is refused — then the data gradient on the
 * mode-1 image (sr_conv3x3_f32's direct kernels) with the activation mask as its epilogue: conv2's is masked by the saved ReLU
 * output with slope 0; conv1's gets the identity path of the block as res1 and, in block 0, the saved first-conv output as mask
 * with slope 0.1.  With num_block = 0 that mask has no conv to ride on and is one sr_cb8_relu_mask_f32 launch.  With accumulate
 * every gradient is ADDED to its target: a weight shared by the steps of a branch gets its sum in step order.
 * Launches, exactly: 1 + 2 * num_block data-gradient launches (one per conv; the first conv's only with din), one mask launch
 * more when num_block = 0, and one weight-gradient call per conv with a target (1 + 2 * num_block with everything asked for), each
 * the tile launches and the two-stage reduction of that entry point.  Nothing allocates or synchronises; no atomics: bit-reproducible.  Summation orders and bounds are those of the two
 * existing entry points. */
int sr_vsr_trunk_bwd_f32(const sr_vsr_trunk_cfg* cfg, const sr_vsr_trunk_bwd_desc* d, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_VSR_BWD_H */
