/* libsr_hip.so — the deterministic adjoint of BasicVSR's propagation step input, fp32 on gfx950: the step-input adjoint of
 * sr_hip_vsr_bwd.h (its "atomic entry point" below) with a dprev sum that does not depend on the order in which the adds arrive.
 *
 * Declared apart from sr_hip_vsr_bwd.h so that that header and its ledger stay as they are; everything here uses the types and
 * status codes of sr_hip.h, that header's descriptor and the CB8 layout [N][C/8][H][W][8]; a "window" is a run of channel blocks
 * inside a wider CB8 tensor.  Launch-profiler ids 180, 181, 182 (sr_kernel_name); 179 stays unnamed.  Bad arguments return
 * SR_EINVAL, a short workspace SR_ENOSPACE, with a message in sr_last_error before anything is launched. */
#ifndef SR_HIP_VSR_DET_H
#define SR_HIP_VSR_DET_H

#include "sr_hip.h"
#include "sr_hip_vsr_bwd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Same adjoint, same inputs, same rules as the atomic entry point: g, prev and dprev are CB8 windows of fb blocks, flow and dflow
 * are two planes per image, dprev is ADDED into and dflow is stored, either may be NULL (not both).  The sample position, the cell
 * and the fractions are the forward's bit for bit; a corner outside the image is neither read nor written; a pixel whose position
 * is not finite or lies outside (-1, W) x (-1, H) gets dflow = 0 and adds nothing.
 *
 * dflow is computed exactly as by the atomic entry point — the float64 gather, a lane's terms in block order, the eight lanes of a
 * pixel as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), one rounding to fp32 — and equals its dflow bit for bit.
 *
 * dprev is summed in 64-bit integers.  Per image:
 *   M  = max |g| over the image's window, taken as an unsigned maximum of the bit patterns with the sign cleared (kernel 180), so
 *        it does not depend on the order and a NaN or an Inf shows as bits >= 0x7f800000;
 *   e  = ilogb(M) + 1,  L = ceil(log2(4 * h * w)),  k = 61 - e - L;
 *   a contribution is the float64 term the atomic entry point forms before its single rounding, (double)g * wq with wq the float64
 *        product of (1 - fy) or fy and (1 - fx) or fx; a corner outside the image and a zero wq are skipped;
 *   the term becomes llrint(ldexp(term, k)) (round to nearest even) and is added with a 64-bit integer atomic to an int64
 *        accumulator shaped like the window, [n][fb][h][w][8], in the workspace (kernel 181, which also computes dflow);
 *   kernel 182 writes dprev = (float)((double)dprev + ldexp((double)acc, -k)).
 * Integer addition is associative: the result is bit-reproducible and independent of the launch geometry, of the arrival order and
 * of the other images of the batch.  |term * 2^k| <= 2^(61 - L) and an element has at most h * w <= 2^(L - 2) contributions, so
 * |acc| <= 2^59: no sum overflows.
 *
 * An image with M == 0 leaves its dprev window untouched.  An image whose g holds a NaN or an Inf gets NaN in every element of its
 * dprev window (the failure stays visible, as with float adds); its dflow is what the gather computes.
 *
 * Bound, with d contributions to an element and `before` what dprev held:
 *   |dprev - (before + exact)| <= 2^-24 |before + exact| + d * 2^-(k + 1) + 2^-50 * sum |terms|
 * the first term is the single rounding to fp32, the second the rounding of each term to a multiple of 2^-k, the third the float64
 * products, the conversion of the accumulator and the float64 add.  The second term: d <= h * w <= 2^(L - 2) and 2^e <= 2 M, so
 * d * 2^-(k + 1) = d * 2^(e + L - 62) <= M * 2^(2 L - 63), reached only where every pixel of the image samples one cell; with
 * d <= 4 contributions (a smooth flow) it is at most M * 2^(L - 59).  For h * w <= 2^16 (L <= 18) the worst case is M * 2^-27,
 * an eighth of an fp32 ulp of M.
 *
 * Workspace: the accumulators, roundup256(64 * n * fb * h * w) bytes, then one scale word per image, roundup256(4 * n) bytes;
 * sr_vsr_prop_input_bwd_det_workspace_bytes is their sum, 0 for a bad shape (n * fb * h * w above 2^50 is one).  The workspace is
 * needed (and cleared, by a stream-ordered memset) only when dprev is given; with dprev NULL it may be NULL and only kernel 181 is
 * launched.  With dprev: kernels 180, 181, 182 in that order.  Nothing allocates or synchronises. */
size_t sr_vsr_prop_input_bwd_det_workspace_bytes(int n, int h, int w, int fb);

typedef struct sr_vsr_prop_bwd_det_desc {
  sr_vsr_prop_bwd_desc d;          /* as for the atomic entry point: same alignment, stride, shape and overlap rules */
  void* workspace;                 /* sr_vsr_prop_input_bwd_det_workspace_bytes bytes, 256-byte aligned; may be NULL with d.dprev NULL */
  size_t workspace_bytes;
} sr_vsr_prop_bwd_det_desc;
int sr_vsr_prop_input_bwd_det_f32(const sr_vsr_prop_bwd_det_desc* d, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_VSR_DET_H */
