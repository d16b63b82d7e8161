// The deterministic step-input adjoint of BasicVSR on gfx950, fp32 on CB8 (include/sr_hip_vsr_det.h): the adjoint of vsr_bwd_ops.hip
// with the dprev sum taken in 64-bit integers (fixed_sum.h), so that it does not depend on the order in which the adds arrive.
//
// Three kernels per call.  The scale kernel takes, per image, the unsigned maximum of the sign-cleared bit patterns of g (one
// wave reduction, then one integer atomic per wave: order-free).  The scatter kernel is the atomic one's body (vsr_prop_bwd.h) —
// dflow is the same float64 gather with the same eight-lane tree — but a dprev term is scaled by 2^k, rounded to an integer and
// added with one 64-bit integer atomic per corner into the workspace: a wave instruction adds eight 64-byte runs.  The finish
// kernel adds the scaled-back sums into dprev with one rounding.  No LDS.
#include <math.h>

#include <algorithm>

#include "../../include/sr_hip_vsr_det.h"
#include "fixed_sum.h"
#include "sr_internal.h"
#include "vsr_prop_bwd.h"

namespace {

using vsrprop::DetParams;

// grid (blocks, n), 256 threads: a grid-stride walk over the window of one image, 16 bytes a lane
__global__ __launch_bounds__(256) void vsr_prop_det_scale_kernel(const DetParams p) {
  const int n = blockIdx.y;
  const long long quads = (long long)p.H * p.W * 2 * p.fb;  // the window of an image is contiguous: fb * H * W * 8 floats
  const unsigned m = fixsum::walk_max((const uint4*)(p.g + (long long)n * p.g_ns), quads);
  fixsum::publish_max(p.scale + n, fixsum::wave_max(m));
}

__global__ __launch_bounds__(256) void vsr_prop_det_scatter_kernel(const DetParams p) { vsrprop::input_bwd_body<true>(p); }

// grid (ceil(fb * HW * 8 / 256), n), 256 threads: one element of the window a lane
__global__ __launch_bounds__(256) void vsr_prop_det_finish_kernel(const DetParams p) {
  const int n = blockIdx.y;
  const long long win = (long long)p.fb * p.H * p.W * 8;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned mbits = p.scale[n];
  if (i >= win || mbits == 0u) return;
  float* d = p.dprev + (long long)n * p.dprev_ns + i;
  if (mbits >= fixsum::kInfBits) {
    *d = __builtin_nanf("");
    return;
  }
  *d = (float)((double)*d + fixsum::scaled_back(p.acc[(long long)n * win + i], vsrprop::scale_shift(mbits, p.L)));
}

// the carve of the workspace; false for a bad shape
bool det_sizes(int n, int h, int w, int fb, fixsum::Carve* c) {
  if (n <= 0 || n > 65535 || h <= 0 || w <= 0 || fb <= 0 || fb >= 65535) return false;
  const long long hw = (long long)h * w;
  if (hw >= (1ll << 28)) return false;
  const unsigned long long elems = (unsigned long long)n * (unsigned long long)fb * (unsigned long long)hw;  // < 2^60: no wrap
  if (elems > (1ull << 50)) return false;  // 64 bytes an element would pass 2^56: no such workspace, and the size must not wrap
  *c = fixsum::carve((size_t)64 * (size_t)elems, (size_t)4 * (size_t)n);
  return true;
}

}  // namespace

extern "C" size_t sr_vsr_prop_input_bwd_det_workspace_bytes(int n, int h, int w, int fb) {
  fixsum::Carve c;
  return det_sizes(n, h, w, fb, &c) ? c.total() : 0;
}

extern "C" int sr_vsr_prop_input_bwd_det_f32(const sr_vsr_prop_bwd_det_desc* dd, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "sr_vsr_prop_input_bwd_det_f32";
  SR_CHECK_ARG(dd != nullptr, "%s: null descriptor", who);
  const sr_vsr_prop_bwd_desc* d = &dd->d;
  DetParams p = {};
  if (int rc = vsrprop::check_and_fill(who, d, (1ll << 38) - 1, &p)) return rc;
  const long long hw = (long long)d->h * d->w, win = hw * 8 * d->fb;
  fixsum::Carve c;
  SR_CHECK_ARG(det_sizes(d->n, d->h, d->w, d->fb, &c), "%s: bad shape n=%d h=%d w=%d fb=%d", who, d->n, d->h, d->w, d->fb);
  p.L = fixsum::level_of(4 * hw);
  if (d->dprev) {
    if (int rc = fixsum::check_and_clear(who, "sr_vsr_prop_input_bwd_det_workspace_bytes", dd->workspace, dd->workspace_bytes, c, stream))
      return rc;
    p.acc = (long long*)dd->workspace;
    p.scale = (unsigned*)((char*)dd->workspace + c.acc_bytes);
  }
  const bool prof = sr::prof_on();
  const int c8 = 8 * d->fb;
  const double px = (double)d->n * (double)hw, ch = c8;
  if (d->dprev) {
    const long long quads = hw * 2 * d->fb;
    const unsigned blocks = (unsigned)std::min<long long>((quads + 255) / 256, 1024);
    if (prof) sr::prof_rec(stream, 180, c8, c8, d->n, d->h, d->w, px * ch, px * ch * 4.0);
    hipLaunchKernelGGL(vsr_prop_det_scale_kernel, dim3(blocks, (unsigned)d->n), dim3(256), 0, stream, p);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_vsr_prop_input_bwd_det_f32 scale launch");
  }
  // per pixel and channel: g once; dflow: four corner reads and 14 float64 operations; dprev: four 8-byte read-modify-writes
  if (prof)
    sr::prof_rec(stream, 181, c8, c8, d->n, d->h, d->w, px * ch * ((d->dflow ? 14.0 : 0.0) + (d->dprev ? 12.0 : 0.0)),
                 px * (ch * (4.0 + (d->dflow ? 16.0 : 0.0) + (d->dprev ? 64.0 : 0.0)) + 8.0 + (d->dflow ? 8.0 : 0.0)));
  hipLaunchKernelGGL(vsr_prop_det_scatter_kernel, dim3((unsigned)((hw + 31) / 32), (unsigned)d->n), dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_vsr_prop_input_bwd_det_f32 scatter launch");
  if (d->dprev) {
    if (prof) sr::prof_rec(stream, 182, c8, c8, d->n, d->h, d->w, px * ch * 2.0, px * ch * 16.0);
    hipLaunchKernelGGL(vsr_prop_det_finish_kernel, dim3((unsigned)((win + 255) / 256), (unsigned)d->n), dim3(256), 0, stream, p);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_vsr_prop_input_bwd_det_f32 finish launch");
  }
  return SR_OK;
}
