// The deterministic input gradient of the modulated deformable convolution on gfx950, fp32 on CB8 (include/sr_hip_dcn_det.h): the dx
// of dcn_ops.hip's dcn_bwd_data_kernel with the sum taken in 64-bit integers, so that it does not depend on the order in which the
// adds arrive (fixed_sum.h).  doffset and dmask come from that kernel itself, launched without dx.
//
// Three kernels per call.  The scale kernel takes, per image, the unsigned maxima of the sign-cleared bit patterns of dcol and of the
// mask (one wave reduction, then one integer atomic per wave: order-free).  The scatter kernel has one lane per element of dcol — a
// lane is (pixel, channel e of a block) of one (tap, block), the channel fastest — which forms its four float64 terms, scales them
// by 2^k, rounds them to integers and adds each with one 64-bit integer atomic into the workspace: a wave instruction adds eight
// 64-byte runs.  It has no loop: taps and blocks are blockIdx.y.  The finish kernel stores the scaled-back sums with one rounding.
// No LDS.
#include <math.h>

#include <algorithm>

#include "../../include/sr_hip_dcn_det.h"
#include "dcn_device.h"
#include "fixed_sum.h"
#include "sr_internal.h"

namespace {

struct DcnDetParams {
  const float* dcol;
  const float* off;
  const float* msk;
  float* dx;
  long long* acc;        // [n][cin_blocks][H][W][8]
  unsigned* scale;       // [n][2]: max over the image of the bits of |dcol|, of |mask|
  long long off_ns, msk_ns, dx_ns;
  int H, W, cin_blocks, bpg, dg, logit, L;
};

using fixsum::exp_of;
using fixsum::kInfBits;

// What the image's two scale words say: 0 = dx is zero, 1 = dx is NaN, 2 = sum with the shift k
__device__ __forceinline__ int scale_state(unsigned md, unsigned mm, int logit, int L, int& k) {
  k = 0;
  if (md >= kInfBits || mm >= kInfBits) return 1;  // with a logit mask mm is 0 or the bits of a NaN
  if (md == 0u || (!logit && mm == 0u)) return 0;
  k = 61 - (exp_of(md) + (logit ? 0 : exp_of(mm))) - L;
  return 2;
}

// grid (blocks, n), 256 threads: a grid-stride walk over the image's dcol (contiguous, 16 bytes a lane), then over its mask blocks
__global__ __launch_bounds__(256) void deform_det_scale_kernel(const DcnDetParams p) {
  const int n = blockIdx.y;
  const long long HW = (long long)p.H * p.W;
  const long long quads = HW * 2 * 9 * p.cin_blocks;
  const unsigned md = fixsum::walk_max((const uint4*)(p.dcol + (long long)n * quads * 4), quads);
  unsigned mm = 0;
  const int mch = 9 * p.dg;  // the pad channels of the last mask block are not the mask's
  const long long melems = (long long)((mch + 7) / 8) * HW * 8;
  const unsigned* mp = (const unsigned*)(p.msk + (long long)n * p.msk_ns);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < melems; i += (long long)gridDim.x * 256) {
    const int c = (int)(i / (HW * 8)) * 8 + (int)(i & 7);
    if (c < mch) {
      const unsigned v = mp[i] & 0x7fffffffu;
      if (!p.logit || v > kInfBits) mm = max(mm, v);
    }
  }
  const unsigned wd = fixsum::wave_max(md), wm = fixsum::wave_max(mm);
  fixsum::publish_max(p.scale + 2 * n, wd);
  fixsum::publish_max(p.scale + 2 * n + 1, wm);
}

// grid (ceil(HW / 32), 9 * cin_blocks, n), 256 threads: thread = 8 * (pixel of the workgroup) + channel of the block;
// blockIdx.y = tap * cin_blocks + block, which is also the block of dcol
__global__ __launch_bounds__(256) void deform_det_scatter_kernel(const DcnDetParams p) {
  const int HW = p.H * p.W;
  const int e = threadIdx.x & 7;
  const int pix = blockIdx.x * 32 + (threadIdx.x >> 3);
  const int tb = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  int k;
  if (scale_state(p.scale[2 * n], p.scale[2 * n + 1], p.logit, p.L, k) != 2) return;
  const int tap = tb / p.cin_blocks, cb = tb - tap * p.cin_blocks, g = cb / p.bpg;
  const int y = pix / p.W, x = pix - y * p.W;
  const float* off_n = p.off + (long long)n * p.off_ns;
  const int oc = 18 * g + 2 * tap;
  const float oh = dcndev::channel_at(off_n, HW, pix, oc), ow = dcndev::channel_at(off_n, HW, pix, oc + 1);
  const float m = dcndev::mask_value(dcndev::channel_at(p.msk + (long long)n * p.msk_ns, HW, pix, 9 * g + tap), p.logit);
  const dcndev::Bilinear b = dcndev::tap_position(y, x, tap, oh, ow, p.H, p.W);  // the forward's position, bit for bit
  const float d = p.dcol[(((long long)n * 9 * p.cin_blocks + tb) * HW + pix) * 8 + e];
  const double dm = (double)d * (double)m;  // exact
  const double lh = b.lh, lw = b.lw, hh = 1.0 - lh, hw = 1.0 - lw;  // not b.hh / b.hw, which are rounded to fp32
  const double w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
  // the corner's element; formed only from a valid corner's (hl, wl)
  unsigned long long* ap = (unsigned long long*)p.acc + ((long long)n * p.cin_blocks + cb) * HW * 8 + e;
  const long long corner = ((long long)b.hl * p.W + b.wl) * 8, down = (long long)p.W * 8;
  if (b.v1 && w1 != 0.0) fixsum::add_term(ap + corner, dm * w1, k);  // |t| <= 2^(61 - L)
  if (b.v2 && w2 != 0.0) fixsum::add_term(ap + corner + 8, dm * w2, k);
  if (b.v3 && w3 != 0.0) fixsum::add_term(ap + corner + down, dm * w3, k);
  if (b.v4 && w4 != 0.0) fixsum::add_term(ap + corner + down + 8, dm * w4, k);
}

// grid (ceil(cin * HW / 256), n), 256 threads: one element of dx a lane
__global__ __launch_bounds__(256) void deform_det_finish_kernel(const DcnDetParams p) {
  const int n = blockIdx.y;
  const long long img = (long long)p.cin_blocks * p.H * p.W * 8;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= img) return;
  int k;
  const int state = scale_state(p.scale[2 * n], p.scale[2 * n + 1], p.logit, p.L, k);
  float v = 0.f;
  if (state == 1) v = __builtin_nanf("");
  if (state == 2) v = (float)fixsum::scaled_back(p.acc[(long long)n * img + i], k);
  p.dx[(long long)n * p.dx_ns + i] = v;
}

// the carve of the workspace; false for a bad shape
bool det_sizes(int n, int cin, int h, int w, fixsum::Carve* c) {
  if (n <= 0 || n > 65535 || cin <= 0 || cin % 8 || 9 * (cin / 8) > 65535 || h <= 0 || w <= 0) return false;
  const long long hw = (long long)h * w;  // < 2^62
  if (hw >= (1ll << 32) || 9ll * cin * hw * 4 >= (1ll << 32)) return false;  // the atomic entry point's "image too large"
  *c = fixsum::carve((size_t)8 * (size_t)n * (size_t)cin * (size_t)hw, (size_t)8 * (size_t)n);  // < 8 * 2^16 * 2^27
  return true;
}

}  // namespace

extern "C" size_t sr_dcn_bwd_data_det_workspace_bytes(int n, int cin, int h, int w) {
  fixsum::Carve c;
  return det_sizes(n, cin, h, w, &c) ? c.total() : 0;
}

extern "C" int sr_dcn_bwd_data_det_f32(const sr_dcn_bwd_det_desc* dd, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "sr_dcn_bwd_data_det_f32";
  SR_CHECK_ARG(dd != nullptr, "%s: null descriptor", who);
  const sr_dcn_bwd_desc* b = &dd->d;
  const sr_dcn_desc* d = &b->fwd;
  {  // the atomic entry point's own checks of the forward descriptor and of dcol; with no destination it launches nothing
    sr_dcn_bwd_desc probe = *b;
    probe.dx = probe.doffset = probe.dmask = nullptr;
    if (int rc = sr_dcn_bwd_data_f32(&probe, stream_)) return rc;
  }
  SR_CHECK_ARG((b->doffset == nullptr) == (b->dmask == nullptr), "%s: doffset and dmask go together", who);
  SR_CHECK_ARG(((uintptr_t)b->dx | (uintptr_t)b->doffset | (uintptr_t)b->dmask) % 16 == 0, "%s: pointers must be 16-byte aligned", who);
  if (!b->dx && !b->doffset) return SR_OK;
  const long long hw = (long long)d->h * d->w;
  if (b->dx) {
    fixsum::Carve c;
    SR_CHECK_ARG(det_sizes(d->n, d->cin, d->h, d->w, &c), "%s: bad shape n=%d cin=%d h=%d w=%d", who, d->n, d->cin, d->h, d->w);
    SR_CHECK_ARG(b->dx_img_stride % 4 == 0, "%s: the image stride of dx must be a multiple of 4 floats", who);
    SR_CHECK_ARG(d->n == 1 || b->dx_img_stride >= (long long)d->cin * hw, "%s: the image stride of dx is smaller than the image", who);
    SR_CHECK_ARG((const float*)b->dx != d->x && (const float*)b->dx != b->dcol, "%s: dx must not be a source", who);
    if (int rc = fixsum::check_and_clear(who, "sr_dcn_bwd_data_det_workspace_bytes", dd->workspace, dd->workspace_bytes, c, stream)) return rc;
    DcnDetParams p = {};
    p.dcol = b->dcol;
    p.off = d->offset;
    p.msk = d->mask;
    p.dx = b->dx;
    p.acc = (long long*)dd->workspace;
    p.scale = (unsigned*)((char*)dd->workspace + c.acc_bytes);
    p.off_ns = d->offset_img_stride;
    p.msk_ns = d->mask_img_stride;
    p.dx_ns = b->dx_img_stride;
    p.H = d->h;
    p.W = d->w;
    p.cin_blocks = d->cin / 8;
    p.bpg = d->cin / d->deformable_groups / 8;
    p.dg = d->deformable_groups;
    p.logit = d->mask_is_logit;
    p.L = fixsum::level_of(9 * hw);
    const bool prof = sr::prof_on();
    const double px = (double)d->n * (double)hw, ch = d->cin;
    const long long quads = hw * 2 * 9 * p.cin_blocks;
    const unsigned blocks = (unsigned)std::min<long long>((quads + 255) / 256, 1024);
    if (prof) sr::prof_rec(stream, 184, d->cin, d->cout, d->n, d->h, d->w, px * (9.0 * ch + 9.0 * p.dg), 4.0 * px * (9.0 * ch + 9.0 * p.dg));
    hipLaunchKernelGGL(deform_det_scale_kernel, dim3(blocks, (unsigned)d->n), dim3(256), 0, stream, p);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_dcn_bwd_data_det_f32 scale launch");
    // per element of dcol: itself, two offsets and a mask value, nine float64 operations, four 8-byte read-modify-writes
    if (prof) sr::prof_rec(stream, 185, d->cin, d->cout, d->n, d->h, d->w, px * 9.0 * ch * 12.0, px * 9.0 * ch * (4.0 + 12.0 + 64.0));
    hipLaunchKernelGGL(deform_det_scatter_kernel, dim3((unsigned)((hw + 31) / 32), (unsigned)(9 * p.cin_blocks), (unsigned)d->n), dim3(256), 0,
                       stream, p);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_dcn_bwd_data_det_f32 scatter launch");
    if (prof) sr::prof_rec(stream, 186, d->cin, d->cout, d->n, d->h, d->w, px * ch * 2.0, px * ch * 12.0);
    hipLaunchKernelGGL(deform_det_finish_kernel, dim3((unsigned)(((long long)d->cin * hw + 255) / 256), (unsigned)d->n), dim3(256), 0, stream,
                       p);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_dcn_bwd_data_det_f32 finish launch");
  }
  if (b->doffset) {  // the gather of the atomic entry point, unchanged: its kernel without dx
    sr_dcn_bwd_desc gather = *b;
    gather.dx = nullptr;
    return sr_dcn_bwd_data_f32(&gather, stream_);
  }
  return SR_OK;
}
