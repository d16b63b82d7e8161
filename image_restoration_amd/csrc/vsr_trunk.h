// What vsr_bwd_ops.hip (include/sr_hip_vsr_bwd.h) shares of the trunk driver in vsr_ops.hip (include/sr_hip_vsr.h): the driver
// itself, so that the training forward issues the launches of the inference forward and not a copy of them.
#pragma once
#include "../../include/sr_hip_vsr.h"
#include "sr_internal.h"

namespace sr {

// Bytes of one activation buffer of a trunk call (num_feat channels of n images, rounded up to 256); 0 for a bad config or shape.
size_t vsr_trunk_act_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w);
// The fp32 trunk call with every activation kept: activation i (0 the first conv's output, 1 + 2 b the ReLU output of block b,
// 2 + 2 b the output of block b < num_block - 1) goes to buffer i of `stack`, 2 * num_block buffers of vsr_trunk_act_bytes.
int vsr_trunk_keep_run(const sr_vsr_trunk_cfg* cfg, const char* who, const char* stack_query, const float* packed, const float* in,
                       long long in_img_stride, float* out, long long out_img_stride, int n, int h, int w, void* stack,
                       size_t stack_bytes, hipStream_t stream);

}  // namespace sr
