/* libsr_hip.so — the segmented Adam step: torch.optim.Adam over one fp32 arena whose parameters fall into classes with their
 * own learning rate, their own bias-correction step count, or no update at all (frozen parameters).
 *
 * Declared apart from sr_hip.h so that the existing ABI header and its ledger stay as they are; everything here uses the
 * types and status codes of sr_hip.h.  Launch-profiler id 139 (sr_kernel_name); 138 stays unnamed.
 * fp32, no atomics, no LDS, no scratch, bit-reproducible.  Bad arguments return SR_EINVAL with a message in sr_last_error
 * before anything is launched. */
#ifndef SR_HIP_TRAIN_GROUPS_H
#define SR_HIP_TRAIN_GROUPS_H

#include "sr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SR_ADAM_MAX_CLASSES 16
#define SR_ADAM_CHUNK 64 /* floats per entry of class_of_chunk: the alignment of a parameter inside the arena */

/* One class of arena chunks: what torch.optim.Adam keeps per parameter group (lr) and per parameter (step), plus whether
 * the chunk takes part in this step at all.  `step` is the count INCLUDING this step (>= 1 when active, as the `step` of
 * sr_adam_step_f32); it is not looked at when active == 0. */
typedef struct sr_adam_class {
  float lr;
  int step;
  int active;
} sr_adam_class;

/* One Adam step over param / grad / exp_avg / exp_avg_sq [n] in one launch.
 *
 *   n               a multiple of SR_ADAM_CHUNK; the four arrays are 16-byte aligned.
 *   class_of_chunk  DEVICE array of n / SR_ADAM_CHUNK bytes: the class of floats [64 k, 64 k + 64).  The caller rewrites it
 *                   only when the partition changes.
 *   classes         HOST array of n_classes (1 .. SR_ADAM_MAX_CLASSES) entries.  The entry point derives each class's
 *                   1 - beta1^step and sqrt(1 - beta2^step) in double, as sr_adam_step_f32 does, and hands the table to the
 *                   kernel BY VALUE in its arguments: no copy to the device and no synchronisation per step.
 *
 * Elements of a chunk whose class is inactive are neither read nor written: parameter, both moments and the gradient slot
 * stay as they are, whatever they hold (NaN in a frozen parameter's gradient slot is harmless).  A class id >= n_classes
 * cannot be seen from the host, which never reads class_of_chunk: the kernel treats such a chunk as inactive.
 *
 * Per element the arithmetic is the operation sequence of sr_adam_step_f32, built with the same contraction flags: a call
 * whose chunks all belong to one active class with the same lr and step gives the bits of sr_adam_step_f32.
 *
 * abort_word / skipped: as sr_adam_step_f32.  If abort_word is given and the word is non-zero nothing changes and *skipped
 * (if given) is incremented by one: once per call, not once per class.
 *
 * SR_EINVAL: a null param / grad / exp_avg / exp_avg_sq / class_of_chunk / classes, a misaligned array, n <= 0 or not a
 * multiple of SR_ADAM_CHUNK, n_classes outside 1 .. SR_ADAM_MAX_CLASSES, an active class with step < 1. */
int sr_adam_step_groups_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                            const uint8_t* class_of_chunk, const sr_adam_class* classes, int n_classes, float beta1,
                            float beta2, float eps, float weight_decay, float grad_scale, const int32_t* abort_word,
                            int32_t* skipped, void* stream);

/* Host only: the table sr_adam_step_groups_f32 hands to its kernel for these classes, entry by entry into four arrays of
 * n_classes: lr, 1 - beta1^step, sqrt(1 - beta2^step) (both rounded from double) and active (0 / 1).  An inactive class
 * reads lr 0, corrections 1.  The same refusals for classes / n_classes / step; the outputs must not be null. */
int sr_adam_class_table(const sr_adam_class* classes, int n_classes, float beta1, float beta2, float* lr, float* bc1,
                        float* bc2_sqrt, int* active);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_TRAIN_GROUPS_H */
