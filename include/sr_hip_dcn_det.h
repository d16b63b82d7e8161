/* libsr_hip.so — the deterministic input gradient of the modulated deformable convolution, fp32 on gfx950: sr_dcn_bwd_data_f32 of
 * sr_hip_dcn.h (its "atomic entry point" below) with a dx that does not depend on the order in which the adds arrive.
 *
 * Declared apart from sr_hip_dcn.h so that that header and its ledger stay as they are; everything here uses the types and status
 * codes of sr_hip.h, that header's descriptors and the CB8 layout [N][C/8][H][W][8].  Launch-profiler ids 184, 185, 186
 * (sr_kernel_name); 183 stays unnamed.  Bad arguments return SR_EINVAL, a short workspace SR_ENOSPACE, with a message in
 * sr_last_error before anything is launched. */
#ifndef SR_HIP_DCN_DET_H
#define SR_HIP_DCN_DET_H

#include "sr_hip.h"
#include "sr_hip_dcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Same gradients, same inputs, same rules as the atomic entry point: `fwd` gives x, offset, mask, mask_is_logit and the geometry,
 * dcol is the CB8 column gradient of 9 * cin channels (tap-major, image stride 9 * cin * h * w), any of dx / doffset / dmask may
 * be NULL, doffset and dmask go together.  The descriptor is first checked by the atomic entry point's own rules (a message of
 * those rules carries that entry point's name), then by the rules of dx below.
 *
 * doffset and dmask are written by the atomic entry point's kernel (id 112) launched without dx: they equal its bit for bit.
 *
 * dx is STORED, not added into: the caller need not zero it, and every element of the cin channels of every image is written.
 * It is the exact sum of its terms, rounded once.  Per (image, deformable group g, tap, pixel) the sampling position, the cell
 * (floor) and the `inside` test are the forward's bit for bit (fp32); lh and lw are its fp32 fractions.  For a channel c of the
 * group and each of the four corners that lies in the image (and only inside the `inside` test)
 *   term = ((double)dcol_c * (double)m) * wq,   wq = (1 - lh or lh) * (1 - lw or lw) in float64 from the fp32 fractions,
 * m the fp32 mask value (after the fp32 sigmoid of the forward for a logit mask).  (double)dcol * (double)m is exact; 1 - lh, 1 - lw,
 * wq and the term are one float64 operation each; nothing is rounded to fp32.  A term whose wq is zero is skipped.
 *
 * The sum is taken in 64-bit integers.  Per image:
 *   Md = max |dcol| over the image, Mm = max |mask| over its 9 * dg mask channels, each taken as an unsigned maximum of the bit
 *        patterns with the sign cleared (kernel 184), so neither depends on the order and a NaN or an Inf shows as bits
 *        >= 0x7f800000.  With a logit mask |m| <= 1 and the mask's factor is 1: only a NaN logit (bits > 0x7f800000) is recorded;
 *   e  = ilogb(Md) + 1 + (raw mask: ilogb(Mm) + 1; logit mask: 0), so that |dcol * m| < 2^e;
 *   L  = ceil(log2(9 * h * w)),  k = 61 - e - L;
 *   the term becomes llrint(ldexp(term, k)) (round to nearest even) and is added with a 64-bit integer atomic to an int64
 *        accumulator [n][cin/8][h][w][8] in the workspace (kernel 185: a lane is (pixel, channel of a block) of one (tap, block),
 *        the channel fastest, and issues four atomics and no loop);
 *   kernel 186 stores dx = (float)ldexp((double)acc, -k).
 * Integer addition is associative: dx is bit-reproducible and independent of the launch geometry, of the arrival order and of
 * the other images of the batch.
 *
 * No overflow, for any input: |wq| <= 1 and |dcol * m| < 2^e give |term * 2^k| < 2^(61 - L), so |llrint(...)| <= 2^(61 - L); an
 * element of dx receives at most one term per (pixel, tap) of its group — the four corners of one position are four different
 * elements — so d <= 9 * h * w <= 2^L terms, and |acc| <= 2^61 < 2^63.
 *
 * Md == 0 (or, with a raw mask, Mm == 0) gives dx == 0.  An image whose dcol holds a NaN or an Inf (or whose raw mask does, or
 * whose logit mask holds a NaN) gets NaN in every element of its dx: the failure stays visible, as with float adds.  A position
 * that is not finite fails the `inside` test and contributes nothing, as in the forward.
 *
 * Bound, with d terms to an element:
 *   |dx - exact| <= 2^-24 |exact| + d * 2^-(k + 1) + 2^-50 * sum |terms|
 * the first term is the single rounding to fp32, the second the rounding of each term to a multiple of 2^-k, the third the
 * float64 roundings of a term (1 - lh, 1 - lw, wq and the product: four at most, 2^-53 each, relative) and the conversion of the
 * accumulator to float64 (2^-53 of at most the sum of |terms| plus the second term).  The second term: d <= 9 h w <= 2^L and 2^e <= 2 Md * 2 Mm (2 Md for a logit mask), so
 * d * 2^-(k + 1) = d * 2^(e + L - 62) <= 4 Md Mm * 2^(2 L - 62), reached only where every pixel and tap of the image samples one
 * cell; with d <= 36 terms (offsets that keep the taps apart) it is at most 9 Md Mm * 2^(L - 58).  For h * w <= 2^16 (L <= 20,
 * d <= 9 * 2^16) the worst case is 9 * 2^16 * 4 Md Mm * 2^-42 = 9 * 2^-24 * Md Mm, nine fp32 half-ulps of Md Mm against an exact
 * sum of up to 9 * 2^16 such terms; with d <= 36 it is below Md Mm * 2^-34.
 *
 * Workspace: the accumulators, roundup256(8 * n * cin * h * w) bytes, then two scale words per image (Md, Mm),
 * roundup256(8 * n) bytes; sr_dcn_bwd_data_det_workspace_bytes is their sum, 0 for a bad shape (n above 65535, cin no multiple of
 * 8 or above 8 * 7281, 9 * cin * h * w * 4 bytes at or above 2^32).  The workspace is needed (and cleared, by a stream-ordered
 * memset) only when dx is given; with dx NULL it may be NULL and only kernel 112 is launched.  With dx: kernels 184, 185, 186 in
 * that order, then 112 when doffset / dmask are given.  Nothing allocates or synchronises. */
size_t sr_dcn_bwd_data_det_workspace_bytes(int n, int cin, int h, int w);

typedef struct sr_dcn_bwd_det_desc {
  sr_dcn_bwd_desc d;               /* as for the atomic entry point; dx: 16-byte aligned, image stride a multiple of 4 floats and,
                                      with n > 1, at least cin * h * w; not x, not dcol */
  void* workspace;                 /* sr_dcn_bwd_data_det_workspace_bytes bytes, 256-byte aligned; may be NULL with d.dx NULL */
  size_t workspace_bytes;
} sr_dcn_bwd_det_desc;
int sr_dcn_bwd_data_det_f32(const sr_dcn_bwd_det_desc* d, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SR_HIP_DCN_DET_H */
