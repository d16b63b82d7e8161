// The segmented Adam step (include/sr_hip_train_groups.h): torch.optim.Adam over one arena whose 64-float chunks fall into up
// to 16 classes, each with its own learning rate and bias-correction step count, or frozen.  EDVR's recipe needs it: a second
// parameter group for the deformable convolutions (train.dcn_lr_mul) and a warm-up in which only the fusion module trains
// (train.tsa_iter), after which the parameters carry different step counts.
//
// Memory-bound: 16 bytes read and 12 written per element, plus one byte of class id per 64 floats.  A thread owns 4 consecutive
// floats (one 16-byte load of each of the four arrays, one 16-byte store of three), so a wave moves 1 KiB per access and the
// 16 threads of a chunk read the same class byte, which the memory pipeline serves from one line.  A parameter never shares a
// chunk with another (FlatAdam's alignment), so the class is read once per thread.  The class table (lr, 1 - beta1^t,
// sqrt(1 - beta2^t), active) travels by value in the kernel arguments: the host writes 256 bytes into the launch packet and
// nothing is copied to the device or waited for.  A thread of an inactive chunk returns before it touches any of the four
// arrays.  No LDS, no atomics, no scratch: the table is indexed in the kernel-argument segment.
//
// The arithmetic per element is adam_kernel's (train_ops.hip), operation for operation, built with the same -ffp-contract=off:
// with one active class the result has the bits of sr_adam_step_f32.
#include <math.h>
#include <stdint.h>

#include "sr_internal.h"
#include "../../include/sr_hip_train_groups.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

struct ClassTable {  // by value in the kernel arguments
  float lr[SR_ADAM_MAX_CLASSES];
  float bc1[SR_ADAM_MAX_CLASSES];
  float bc2_sqrt[SR_ADAM_MAX_CLASSES];
  int active[SR_ADAM_MAX_CLASSES];
};

__global__ __launch_bounds__(256) void adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long long n4, const uint8_t* __restrict__ cls,
                                                          const ClassTable tab, int n_classes, float b1, float b2, float eps,
                                                          float wd, float grad_scale, const int32_t* __restrict__ abort_word,
                                                          int32_t* __restrict__ skipped) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // index of this thread's float4
  if (abort_word && *abort_word != 0) {  // a launch of this step timed out: its gradients are invalid, the state stays as it is
    if (i == 0 && skipped) *skipped += 1;
    return;
  }
  if (i >= n4) return;
  const int c = cls[i >> 4];  // 16 float4 per 64-float chunk
  if (c >= n_classes || tab.active[c] == 0) return;
  const float lr = tab.lr[c], bc1 = tab.bc1[c], bc2_sqrt = tab.bc2_sqrt[c];
  const f32x4 g4 = ((const f32x4*)g)[i], p4 = ((const f32x4*)p)[i], m4 = ((const f32x4*)m)[i], v4 = ((const f32x4*)v)[i];
  f32x4 po, mo, vo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float gi = g4[e] * grad_scale;
    const float pi = p4[e];
    if (wd != 0.f) gi += wd * pi;
    const float mi = b1 * m4[e] + (1.f - b1) * gi;
    const float vi = b2 * v4[e] + (1.f - b2) * gi * gi;
    mo[e] = mi;
    vo[e] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    po[e] = pi - (lr / bc1) * (mi / denom);
  }
  ((f32x4*)m)[i] = mo;
  ((f32x4*)v)[i] = vo;
  ((f32x4*)p)[i] = po;
}

// checks the classes and derives the table; the bias corrections in double, as sr_adam_step_f32 has them
int build_table(const char* who, const sr_adam_class* classes, int n_classes, float beta1, float beta2, ClassTable* tab) {
  SR_CHECK_ARG(classes, "%s: null classes", who);
  SR_CHECK_ARG(n_classes >= 1 && n_classes <= SR_ADAM_MAX_CLASSES, "%s: n_classes %d outside 1..%d", who, n_classes,
               SR_ADAM_MAX_CLASSES);
  for (int c = 0; c < SR_ADAM_MAX_CLASSES; ++c) {
    tab->lr[c] = 0.f;
    tab->bc1[c] = 1.f;
    tab->bc2_sqrt[c] = 1.f;
    tab->active[c] = 0;
  }
  for (int c = 0; c < n_classes; ++c) {
    if (!classes[c].active) continue;
    SR_CHECK_ARG(classes[c].step >= 1, "%s: active class %d has step %d < 1", who, c, classes[c].step);
    const double bc1 = 1.0 - pow((double)beta1, classes[c].step), bc2 = 1.0 - pow((double)beta2, classes[c].step);
    tab->lr[c] = classes[c].lr;
    tab->bc1[c] = (float)bc1;
    tab->bc2_sqrt[c] = (float)sqrt(bc2);
    tab->active[c] = 1;
  }
  return SR_OK;
}

}  // namespace

extern "C" int sr_adam_class_table(const sr_adam_class* classes, int n_classes, float beta1, float beta2, float* lr, float* bc1,
                                   float* bc2_sqrt, int* active) {
  SR_CHECK_ARG(lr && bc1 && bc2_sqrt && active, "sr_adam_class_table: null output");
  ClassTable tab;
  const int rc = build_table("sr_adam_class_table", classes, n_classes, beta1, beta2, &tab);
  if (rc != SR_OK) return rc;
  for (int c = 0; c < n_classes; ++c) {
    lr[c] = tab.lr[c];
    bc1[c] = tab.bc1[c];
    bc2_sqrt[c] = tab.bc2_sqrt[c];
    active[c] = tab.active[c];
  }
  return SR_OK;
}

extern "C" int sr_adam_step_groups_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                       const uint8_t* class_of_chunk, const sr_adam_class* classes, int n_classes, float beta1,
                                       float beta2, float eps, float weight_decay, float grad_scale, const int32_t* abort_word,
                                       int32_t* skipped, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && class_of_chunk, "sr_adam_step_groups_f32: null pointer");
  SR_CHECK_ARG(sr::aligned16(param) && sr::aligned16(grad) && sr::aligned16(exp_avg) && sr::aligned16(exp_avg_sq),
               "sr_adam_step_groups_f32: arrays must be 16-byte aligned");
  SR_CHECK_ARG(n > 0 && n % SR_ADAM_CHUNK == 0, "sr_adam_step_groups_f32: n = %lld is not a positive multiple of %d", (long long)n,
               SR_ADAM_CHUNK);
  SR_CHECK_ARG(n / 4 / 256 < 0x7fffffffLL, "sr_adam_step_groups_f32: n = %lld exceeds the grid", (long long)n);
  ClassTable tab;
  const int rc = build_table("sr_adam_step_groups_f32", classes, n_classes, beta1, beta2, &tab);
  if (rc != SR_OK) return rc;
  const long long n4 = n / 4;
  const bool prof = sr::prof_on();
  if (prof) {
    sr_launch_record r = {};
    r.kernel_id = 139;
    r.cin = n_classes;
    r.n = 1;
    r.flops = 14.0 * (double)n;
    r.bytes = 28.0 * (double)n + (double)(n / SR_ADAM_CHUNK);
    sr::prof_begin(stream, r);
  }
  hipLaunchKernelGGL(adam_groups_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, param, grad, exp_avg, exp_avg_sq,
                     n4, class_of_chunk, tab, n_classes, beta1, beta2, eps, weight_decay, grad_scale, abort_word, skipped);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("adam_groups");
  return SR_OK;
}
