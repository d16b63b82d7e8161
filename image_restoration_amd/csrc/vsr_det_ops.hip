// The deterministic step-input adjoint of BasicVSR on gfx950, fp32 on CB8 (include/sr_hip_vsr_det.h): the adjoint of vsr_bwd_ops.hip
// with the dprev sum taken in 64-bit integers, so that it does not depend on the order in which the adds arrive.
//
// Three kernels per call.  The scale kernel takes, per image, the unsigned maximum of the sign-cleared bit patterns of g (one
// wave reduction, then one integer atomic per wave: order-free).  The scatter kernel is shaped like the atomic one — a lane is
// (pixel, channel e of a block), the channel fastest, and walks the fb blocks; dflow is the same float64 gather with the same
// eight-lane tree — but a dprev term is scaled by 2^k, rounded to an integer and added with one 64-bit integer atomic per corner
// into the workspace: a wave instruction adds eight 64-byte runs.  The finish kernel adds the scaled-back sums into dprev with one
// rounding.  No LDS.
#include <math.h>

#include <algorithm>

#include "../../include/sr_hip_vsr_det.h"
#include "flow_device.h"
#include "sr_internal.h"

namespace {

struct PropDetParams {
  const float* g;
  const float* prev;
  const float* flow;
  float* dprev;
  float* dflow;
  long long* acc;        // [n][fb][H][W][8]
  unsigned* scale;       // [n]: max over the image of the bits of |g|
  long long g_ns, prev_ns, flow_ns, dprev_ns, dflow_ns;
  int H, W, fb, L;
};

constexpr unsigned kInfBits = 0x7f800000u;

// k = 61 - e - L with e = ilogb(M) + 1, from the bits of M (finite, not zero; a denormal has its exponent from its leading bit)
__device__ __forceinline__ int scale_shift(unsigned mbits, int L) {
  const int ex = (int)(mbits >> 23);
  const int ilog = ex ? ex - 127 : (31 - __clz((int)mbits)) - 149;
  return 61 - (ilog + 1) - L;
}

// grid (blocks, n), 256 threads: a grid-stride walk over the window of one image, 16 bytes a lane
__global__ __launch_bounds__(256) void vsr_prop_det_scale_kernel(const PropDetParams p) {
  const int n = blockIdx.y;
  const long long quads = (long long)p.H * p.W * 2 * p.fb;  // the window of an image is contiguous: fb * H * W * 8 floats
  const uint4* src = (const uint4*)(p.g + (long long)n * p.g_ns);
  unsigned m = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) {
    const uint4 v = src[i];
    m = max(max(m, v.x & 0x7fffffffu), max(v.y & 0x7fffffffu, max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, s));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(p.scale + n, m);
}

// grid (ceil(HW / 32), n), 256 threads: thread = 8 * (pixel of the workgroup) + channel of the block
__global__ __launch_bounds__(256) void vsr_prop_det_scatter_kernel(const PropDetParams p) {
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
  // the image's scale: nothing is added for an all-zero g (dprev stays) nor for a non-finite one (the finish kernel writes NaN)
  const unsigned mbits = p.dprev ? p.scale[n] : 0u;
  const bool scatter = mbits != 0u && mbits < kInfBits;
  const int k = scatter ? scale_shift(mbits, p.L) : 0;
  double sx = 0.0, sy = 0.0;
  if (ok) {
    const flowdev::Corners c = flowdev::corners(x0, y0, p.H, p.W);
    const double ax = fx, ay = fy;
    const double wq[4] = {(1.0 - ay) * (1.0 - ax), (1.0 - ay) * ax, ay * (1.0 - ax), ay * ax};
    const float* gp = p.g + (long long)n * p.g_ns + (long long)pix * 8 + e;
    const float* src = p.prev + (long long)n * p.prev_ns + e;
    unsigned long long* ap = (unsigned long long*)p.acc + (long long)n * p.fb * HW * 8 + e;
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
            const long long t = llrint(ldexp((double)gv * wq[q], k));  // |t| <= 2^(61 - L)
            atomicAdd(ap + blk + (long long)c.off[q] * 8, (unsigned long long)t);
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

// grid (ceil(fb * HW * 8 / 256), n), 256 threads: one element of the window a lane
__global__ __launch_bounds__(256) void vsr_prop_det_finish_kernel(const PropDetParams p) {
  const int n = blockIdx.y;
  const long long win = (long long)p.fb * p.H * p.W * 8;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned mbits = p.scale[n];
  if (i >= win || mbits == 0u) return;
  float* d = p.dprev + (long long)n * p.dprev_ns + i;
  if (mbits >= kInfBits) {
    *d = __builtin_nanf("");
    return;
  }
  const long long a = p.acc[(long long)n * win + i];
  *d = (float)((double)*d + ldexp((double)a, -scale_shift(mbits, p.L)));
}

// accumulator bytes and scale bytes, each rounded up to 256; false for a bad shape
bool det_sizes(int n, int h, int w, int fb, size_t* acc_bytes, size_t* scale_bytes) {
  if (n <= 0 || n > 65535 || h <= 0 || w <= 0 || fb <= 0 || fb >= 65535) return false;
  const long long hw = (long long)h * w;
  if (hw >= (1ll << 28)) return false;
  const unsigned long long elems = (unsigned long long)n * (unsigned long long)fb * (unsigned long long)hw;  // < 2^60: no wrap
  if (elems > (1ull << 50)) return false;  // 64 bytes an element would pass 2^56: no such workspace, and the size must not wrap
  *acc_bytes = sr::align_up((size_t)64 * (size_t)elems, 256);
  *scale_bytes = sr::align_up((size_t)4 * (size_t)n, 256);
  return true;
}

}  // namespace

extern "C" size_t sr_vsr_prop_input_bwd_det_workspace_bytes(int n, int h, int w, int fb) {
  size_t a = 0, s = 0;
  return det_sizes(n, h, w, fb, &a, &s) ? a + s : 0;
}

extern "C" int sr_vsr_prop_input_bwd_det_f32(const sr_vsr_prop_bwd_det_desc* dd, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "sr_vsr_prop_input_bwd_det_f32";
  SR_CHECK_ARG(dd != nullptr, "%s: null descriptor", who);
  const sr_vsr_prop_bwd_desc* d = &dd->d;
  SR_CHECK_ARG(d->g && d->prev && d->flow, "%s: null g / prev / flow", who);
  SR_CHECK_ARG(d->dprev || d->dflow, "%s: dprev and dflow are both NULL: nothing to compute", who);
  SR_CHECK_ARG(d->n > 0 && d->n <= 65535 && d->h > 0 && d->w > 0 && d->fb > 0 && d->fb < 65535, "%s: bad shape n=%d h=%d w=%d fb=%d", who,
               d->n, d->h, d->w, d->fb);
  const long long hw = (long long)d->h * d->w, win = hw * 8 * d->fb;
  SR_CHECK_ARG(hw < (1ll << 28) && win < (1ll << 38), "%s: image too large for 32-bit plane offsets", who);
  SR_CHECK_ARG(sr::aligned16(d->g) && sr::aligned16(d->prev) && sr::aligned16(d->dprev), "%s: CB8 windows must be 16-byte aligned", who);
  SR_CHECK_ARG(((uintptr_t)d->flow & 3u) == 0 && ((uintptr_t)d->dflow & 3u) == 0, "%s: flow / dflow must be 4-byte aligned", who);
  SR_CHECK_ARG(d->g_img_stride % 4 == 0 && d->prev_img_stride % 4 == 0 && (!d->dprev || d->dprev_img_stride % 4 == 0),
               "%s: image strides of CB8 windows must be multiples of 4 floats", who);
  SR_CHECK_ARG(d->n == 1 || (d->g_img_stride >= win && d->prev_img_stride >= win && d->flow_img_stride >= 2 * hw &&
                             (!d->dprev || d->dprev_img_stride >= win) && (!d->dflow || d->dflow_img_stride >= 2 * hw)),
               "%s: an image stride is smaller than the image", who);
  SR_CHECK_ARG(d->dprev != d->g && d->dprev != d->prev && d->dflow != d->flow, "%s: a destination must not be a source", who);
  size_t acc_bytes = 0, scale_bytes = 0;
  SR_CHECK_ARG(det_sizes(d->n, d->h, d->w, d->fb, &acc_bytes, &scale_bytes), "%s: bad shape n=%d h=%d w=%d fb=%d", who, d->n, d->h, d->w,
               d->fb);
  if (d->dprev) {
    SR_CHECK_ARG(((uintptr_t)dd->workspace & 255u) == 0, "%s: the workspace must be 256-byte aligned", who);
    if (!dd->workspace || dd->workspace_bytes < acc_bytes + scale_bytes) {
      sr::set_error("%s: workspace of %zu bytes, %zu needed (sr_vsr_prop_input_bwd_det_workspace_bytes)", who,
                    dd->workspace ? dd->workspace_bytes : (size_t)0, acc_bytes + scale_bytes);
      return SR_ENOSPACE;
    }
  }
  PropDetParams p = {};
  p.g = d->g;
  p.prev = d->prev;
  p.flow = d->flow;
  p.dprev = d->dprev;
  p.dflow = d->dflow;
  p.g_ns = d->g_img_stride;
  p.prev_ns = d->prev_img_stride;
  p.flow_ns = d->flow_img_stride;
  p.dprev_ns = d->dprev_img_stride;
  p.dflow_ns = d->dflow_img_stride;
  p.H = d->h;
  p.W = d->w;
  p.fb = d->fb;
  p.L = 2;  // ceil(log2(4 * h * w))
  while ((1ll << p.L) < 4 * hw) ++p.L;
  if (d->dprev) {
    p.acc = (long long*)dd->workspace;
    p.scale = (unsigned*)((char*)dd->workspace + acc_bytes);
    if (hipMemsetAsync(dd->workspace, 0, acc_bytes + scale_bytes, stream) != hipSuccess) {
      sr::set_error("%s: clearing the workspace: %s", who, hipGetErrorString(hipGetLastError()));
      return SR_ELAUNCH;
    }
  }
  const bool prof = sr::prof_on();
  const double px = (double)d->n * (double)hw, ch = 8.0 * d->fb;
  auto record = [&](int id, double flops, double bytes) {
    sr_launch_record r = {};
    r.kernel_id = id;
    r.cin = r.cout = 8 * d->fb;
    r.n = d->n;
    r.h = d->h;
    r.w = d->w;
    r.flops = flops;
    r.bytes = bytes;
    sr::prof_begin(stream, r);
  };
  if (d->dprev) {
    const long long quads = hw * 2 * d->fb;
    const unsigned blocks = (unsigned)std::min<long long>((quads + 255) / 256, 1024);
    if (prof) record(180, px * ch, px * ch * 4.0);
    hipLaunchKernelGGL(vsr_prop_det_scale_kernel, dim3(blocks, (unsigned)d->n), dim3(256), 0, stream, p);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_vsr_prop_input_bwd_det_f32 scale launch");
  }
  // per pixel and channel: g once; dflow: four corner reads and 14 float64 operations; dprev: four 8-byte read-modify-writes
  if (prof)
    record(181, px * ch * ((d->dflow ? 14.0 : 0.0) + (d->dprev ? 12.0 : 0.0)),
           px * (ch * (4.0 + (d->dflow ? 16.0 : 0.0) + (d->dprev ? 64.0 : 0.0)) + 8.0 + (d->dflow ? 8.0 : 0.0)));
  hipLaunchKernelGGL(vsr_prop_det_scatter_kernel, dim3((unsigned)((hw + 31) / 32), (unsigned)d->n), dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_vsr_prop_input_bwd_det_f32 scatter launch");
  if (d->dprev) {
    if (prof) record(182, px * ch * 2.0, px * ch * 16.0);
    hipLaunchKernelGGL(vsr_prop_det_finish_kernel, dim3((unsigned)((win + 255) / 256), (unsigned)d->n), dim3(256), 0, stream, p);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_vsr_prop_input_bwd_det_f32 finish launch");
  }
  return SR_OK;
}
