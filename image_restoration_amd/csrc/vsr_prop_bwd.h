// The adjoint of BasicVSR's propagation step input, once: the kernel body and the descriptor checks that the float-atomic entry
// point (vsr_bwd_ops.hip, kernel 178) and the deterministic one (vsr_det_ops.hip, kernel 181) share.
//
// A lane is (pixel, channel e of a block), the channel fastest, and walks the fb blocks: per block it reads one g element, for dflow
// the four corners of prev (gather, float64 accumulator), for dprev it issues four atomics.  A wave instruction therefore covers
// 8 pixels x 8 channels: eight runs per corner, contiguous for neighbouring pixels that sample neighbouring cells (a locally
// constant flow), so the atomics of a wave land in whole lines instead of 64 different ones.  The eight lanes of a pixel add their
// dflow sums through three xor shuffles; lanes past the image stay in the kernel for them and do nothing else.  No LDS.
//
// The two kernels differ in the dprev add alone: a float atomic into dprev itself (32-byte runs), or the term scaled by 2^k and
// added as a 64-bit integer into the workspace (64-byte runs; fixed_sum.h), k from the image's scale word.
#pragma once
#include <type_traits>

#include "../../include/sr_hip_vsr_bwd.h"
#include "fixed_sum.h"
#include "flow_device.h"
#include "sr_internal.h"

namespace vsrprop {

struct Params {
  const float* g;
  const float* prev;
  const float* flow;
  float* dprev;
  float* dflow;
  long long g_ns, prev_ns, flow_ns, dprev_ns, dflow_ns;
  int H, W, fb;
};

struct DetParams : Params {
  long long* acc;   // [n][fb][H][W][8]
  unsigned* scale;  // [n]: max over the image of the bits of |g|
  int L;
};

// k = 61 - e - L with e the exponent of M (finite, not zero)
__device__ __forceinline__ int scale_shift(unsigned mbits, int L) { return 61 - fixsum::exp_of(mbits) - L; }

// grid (ceil(HW / 32), n), 256 threads: thread = 8 * (pixel of the workgroup) + channel of the block
template <bool DET>
__device__ __forceinline__ void input_bwd_body(const std::conditional_t<DET, DetParams, Params>& p) {
  const int HW = p.H * p.W;
  const int e = threadIdx.x & 7;
  const int pix = blockIdx.x * 32 + (threadIdx.x >> 3);
  const int n = blockIdx.y;
  const bool live = pix < HW;
  int x0 = 0, y0 = 0;
  float fx = 0.f, fy = 0.f;
  bool gx_on = false, gy_on = false, ok = false;
  if (live) {
    const int py = pix / p.W, px = pix - py * p.W;
    const float* fl = p.flow + (long long)n * p.flow_ns + pix;
    ok = flowdev::warp_coord(fl[0], fl[HW], px, py, p.H, p.W, /*border=*/0, x0, y0, fx, fy, gx_on, gy_on);
  }
  bool scatter = false;
  int k = 0;
  if constexpr (DET) {
    // the image's scale: nothing is added for an all-zero g (dprev stays) nor for a non-finite one (the finish kernel writes NaN)
    const unsigned mbits = p.dprev ? p.scale[n] : 0u;
    scatter = mbits != 0u && mbits < fixsum::kInfBits;
    k = scatter ? scale_shift(mbits, p.L) : 0;
  }
  double sx = 0.0, sy = 0.0;
  if (ok) {
    const flowdev::Corners c = flowdev::corners(x0, y0, p.H, p.W);
    const double ax = fx, ay = fy;
    const double wq[4] = {(1.0 - ay) * (1.0 - ax), (1.0 - ay) * ax, ay * (1.0 - ax), ay * ax};
    const float* gp = p.g + (long long)n * p.g_ns + (long long)pix * 8 + e;
    const float* src = p.prev + (long long)n * p.prev_ns + e;
    float* dp = nullptr;
    unsigned long long* ap = nullptr;
    if constexpr (DET) {
      ap = (unsigned long long*)p.acc + (long long)n * p.fb * HW * 8 + e;
    } else {
      dp = p.dprev ? p.dprev + (long long)n * p.dprev_ns + e : nullptr;
      scatter = dp != nullptr;
    }
    for (int cb = 0; cb < p.fb; ++cb) {
      const long long blk = (long long)cb * HW * 8;
      const float gv = gp[blk];
      if (p.dflow) {
        const double v00 = c.ok[0] ? src[blk + (long long)c.off[0] * 8] : 0.f, v01 = c.ok[1] ? src[blk + (long long)c.off[1] * 8] : 0.f;
        const double v10 = c.ok[2] ? src[blk + (long long)c.off[2] * 8] : 0.f, v11 = c.ok[3] ? src[blk + (long long)c.off[3] * 8] : 0.f;
        const double gd = gv;
        sx += gd * ((1.0 - ay) * (v01 - v00) + ay * (v11 - v10));
        sy += gd * ((1.0 - ax) * (v10 - v00) + ax * (v11 - v01));
      }
      if (scatter) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c.ok[q] && wq[q] != 0.0) {
            const long long at = blk + (long long)c.off[q] * 8;
            if constexpr (DET)
              fixsum::add_term(ap + at, (double)gv * wq[q], k);  // |t| <= 2^(61 - L)
            else
              atomicAdd(dp + at, (float)((double)gv * wq[q]));  // rounded once
          }
      }
    }
  }
  if (p.dflow) {  // uniform: every lane of the workgroup takes part in the shuffles
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
      sx += __shfl_xor(sx, m);
      sy += __shfl_xor(sy, m);
    }
    if (live && e == 0) {
      float* d = p.dflow + (long long)n * p.dflow_ns + pix;
      d[0] = ok && gx_on ? (float)sx : 0.f;
      d[HW] = ok && gy_on ? (float)sy : 0.f;
    }
  }
}

// The descriptor checks of both entry points and the parameters they share.  max_win: the largest window (fb * h * w * 8 floats)
// the entry point's own offsets allow; the atomic one has no limit beyond that of h * w.
inline int check_and_fill(const char* who, const sr_vsr_prop_bwd_desc* d, long long max_win, Params* p) {
  SR_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  SR_CHECK_ARG(d->g && d->prev && d->flow, "%s: null g / prev / flow", who);
  SR_CHECK_ARG(d->dprev || d->dflow, "%s: dprev and dflow are both NULL: nothing to compute", who);
  SR_CHECK_ARG(d->n > 0 && d->n <= 65535 && d->h > 0 && d->w > 0 && d->fb > 0 && d->fb < 65535, "%s: bad shape n=%d h=%d w=%d fb=%d", who,
               d->n, d->h, d->w, d->fb);
  const long long hw = (long long)d->h * d->w, win = hw * 8 * d->fb;
  SR_CHECK_ARG(hw < (1ll << 28) && win <= max_win, "%s: image too large for 32-bit plane offsets", who);
  SR_CHECK_ARG(sr::aligned16(d->g) && sr::aligned16(d->prev) && sr::aligned16(d->dprev), "%s: CB8 windows must be 16-byte aligned", who);
  SR_CHECK_ARG(((uintptr_t)d->flow & 3u) == 0 && ((uintptr_t)d->dflow & 3u) == 0, "%s: flow / dflow must be 4-byte aligned", who);
  SR_CHECK_ARG(d->g_img_stride % 4 == 0 && d->prev_img_stride % 4 == 0 && (!d->dprev || d->dprev_img_stride % 4 == 0),
               "%s: image strides of CB8 windows must be multiples of 4 floats", who);
  SR_CHECK_ARG(d->n == 1 || (d->g_img_stride >= win && d->prev_img_stride >= win && d->flow_img_stride >= 2 * hw &&
                             (!d->dprev || d->dprev_img_stride >= win) && (!d->dflow || d->dflow_img_stride >= 2 * hw)),
               "%s: an image stride is smaller than the image", who);
  SR_CHECK_ARG(d->dprev != d->g && d->dprev != d->prev && d->dflow != d->flow, "%s: a destination must not be a source", who);
  p->g = d->g;
  p->prev = d->prev;
  p->flow = d->flow;
  p->dprev = d->dprev;
  p->dflow = d->dflow;
  p->g_ns = d->g_img_stride;
  p->prev_ns = d->prev_img_stride;
  p->flow_ns = d->flow_img_stride;
  p->dprev_ns = d->dprev_img_stride;
  p->dflow_ns = d->dflow_img_stride;
  p->H = d->h;
  p->W = d->w;
  p->fb = d->fb;
  return SR_OK;
}

}  // namespace vsrprop
