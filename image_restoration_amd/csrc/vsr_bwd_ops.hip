// The recurrent backward of BasicVSR on gfx950, fp32 on CB8 (include/sr_hip_vsr_bwd.h): the adjoint of the propagation step input,
// the trunk call that keeps its activations (the driver of vsr_ops.hip, through vsr_trunk.h) and the trunk's backward as one C call
// over the existing 3x3 kernels.
//
// The step-input adjoint is one kernel for both gradients: the body of vsr_prop_bwd.h with a float atomic per dprev term.
#include <limits.h>
#include <math.h>

#include <vector>

#include "../../include/sr_hip_ridnet.h"
#include "../../include/sr_hip_vsr_bwd.h"
#include "sr_internal.h"
#include "vsr_prop_bwd.h"
#include "vsr_trunk.h"

namespace {

// ----------------------------------------------------------------------------------- adjoint of the propagation step input
__global__ __launch_bounds__(256) void vsr_prop_input_bwd_kernel(const vsrprop::Params p) { vsrprop::input_bwd_body<false>(p); }

// --------------------------------------------------------------------------------------------------- the trunk's backward
// Channel counts and offsets of the data-gradient images, in state_dict order
struct DgradConv {
  int cout, cin, first_seg, seg, cin_pad;  // the FORWARD conv's
  size_t w_off;
};

struct DgradPlan {
  std::vector<DgradConv> convs;
  size_t packed_bytes;
  int cin_pad0;
};

bool make_dgrad_plan(const sr_vsr_trunk_cfg* c, DgradPlan* P) {
  if (!c || sr_vsr_trunk_packed_bytes(c) == 0) return false;  // the forward's own rule on a config
  size_t off = 0;
  auto add = [&](int cout, int cin, int first_seg, int seg) {
    DgradConv cp;
    cp.cout = cout;
    cp.cin = cin;
    cp.first_seg = first_seg;
    cp.seg = seg;
    cp.cin_pad = sr_conv3x3_cin_pad(cin, first_seg, seg);
    cp.w_off = off;
    // the image convolves dY (cout channels, a multiple of 8 here) into cin_pad channels
    off += sr::align_up(sr_conv3x3_packed_weight_floats(cp.cin_pad, cout) * 4, 256);
    P->convs.push_back(cp);
  };
  const int nf = c->num_feat;
  add(nf, 3 + c->cin_segs * nf, 3, nf);
  for (int b = 0; b < c->num_block; ++b) {
    add(nf, nf, nf, 0);
    add(nf, nf, nf, 0);
  }
  P->cin_pad0 = P->convs[0].cin_pad;
  P->packed_bytes = off;
  return true;
}

#define DGRAD_PLAN(P, cfg, who) \
  SR_CHECK_ARG(make_dgrad_plan(cfg, &P), "%s: bad config (num_feat a multiple of 8, num_block >= 0, cin_segs 1 or 2)", who)

}  // namespace

extern "C" int sr_vsr_prop_input_bwd_f32(const sr_vsr_prop_bwd_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "sr_vsr_prop_input_bwd_f32";
  vsrprop::Params p = {};
  if (int rc = vsrprop::check_and_fill(who, d, LLONG_MAX, &p)) return rc;
  const long long hw = (long long)d->h * d->w;
  const dim3 grid((unsigned)((hw + 31) / 32), (unsigned)d->n);
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * (double)hw, ch = 8.0 * d->fb;
    // per pixel and channel: g once; dflow: four corner reads and 14 float64 operations; dprev: four read-modify-writes
    sr::prof_rec(stream, 178, 8 * d->fb, 8 * d->fb, d->n, d->h, d->w, px * ch * ((d->dflow ? 14.0 : 0.0) + (d->dprev ? 8.0 : 0.0)),
                 px * (ch * (4.0 + (d->dflow ? 16.0 : 0.0) + (d->dprev ? 32.0 : 0.0)) + 8.0 + (d->dflow ? 8.0 : 0.0)));
  }
  hipLaunchKernelGGL(vsr_prop_input_bwd_kernel, grid, dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_vsr_prop_input_bwd_f32 launch");
  return SR_OK;
}

extern "C" size_t sr_vsr_trunk_keep_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w) {
  const size_t one = sr::vsr_trunk_act_bytes(cfg, n, h, w);
  return one ? 2 * (size_t)cfg->num_block * one : 0;
}

extern "C" int sr_vsr_trunk_keep_f32(const sr_vsr_trunk_cfg* cfg, const float* packed, const float* in, long long in_img_stride, float* out,
                                     long long out_img_stride, int n, int h, int w, void* stack, size_t stack_bytes, void* stream) {
  return sr::vsr_trunk_keep_run(cfg, "sr_vsr_trunk_keep_f32", "sr_vsr_trunk_keep_bytes", packed, in, in_img_stride, out, out_img_stride, n,
                                h, w, stack, stack_bytes, (hipStream_t)stream);
}

extern "C" size_t sr_vsr_trunk_packed_dgrad_bytes(const sr_vsr_trunk_cfg* cfg) {
  DgradPlan P;
  if (!make_dgrad_plan(cfg, &P)) return 0;
  return P.packed_bytes + sr::pack_table_bytes(P.convs.size());
}

extern "C" int sr_vsr_trunk_pack_dgrad_f32(const sr_vsr_trunk_cfg* cfg, const float* const* params, float* packed_, void* stream) {
  const char* who = "sr_vsr_trunk_pack_dgrad_f32";
  char* const packed = (char*)packed_;
  DgradPlan P;
  DGRAD_PLAN(P, cfg, who);
  SR_CHECK_ARG(params && packed, "%s: null argument", who);
  SR_CHECK_ARG(((uintptr_t)packed & 255u) == 0, "%s: packed must be 256-byte aligned", who);
  std::vector<sr::PackEntry> tab(P.convs.size());
  for (size_t i = 0; i < P.convs.size(); ++i) {
    const DgradConv& cp = P.convs[i];
    SR_CHECK_ARG(params[2 * i] != nullptr, "%s: null weight %zu", who, i);
    sr::PackEntry& e = tab[i];
    e = sr::PackEntry{};
    e.kind = 1;
    e.w[0] = params[2 * i];
    e.out = packed + cp.w_off;
    e.cout = cp.cout;
    e.cin = cp.cin;
    e.first_seg = cp.first_seg;
    e.seg = cp.seg > 0 ? cp.seg : 1;
    e.cin_pad = cp.cin_pad;
  }
  return sr::pack_table_run(tab, packed, P.packed_bytes, false, (hipStream_t)stream);
}

extern "C" size_t sr_vsr_trunk_bwd_workspace_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w) {
  const size_t one = sr::vsr_trunk_act_bytes(cfg, n, h, w);
  return one ? 3 * one + sr::align_up(sr_conv3x3_wgrad_slab_bytes(n, h, w), 256) : 0;
}

extern "C" int sr_vsr_trunk_bwd_f32(const sr_vsr_trunk_cfg* cfg, const sr_vsr_trunk_bwd_desc* d, void* stream) {
  const char* who = "sr_vsr_trunk_bwd_f32";
  DgradPlan P;
  DGRAD_PLAN(P, cfg, who);
  SR_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  SR_CHECK_ARG(d->packed_dgrad && d->in && d->dout && d->dparams && d->workspace, "%s: null packed_dgrad / in / dout / dparams / workspace", who);
  const int n = d->n, h = d->h, w = d->w, nf = cfg->num_feat, nb = cfg->num_block, fb = nf / 8;
  SR_CHECK_ARG(n > 0 && h > 0 && w > 0, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
  SR_CHECK_ARG(d->accumulate == 0 || d->accumulate == 1, "%s: accumulate must be 0 or 1", who);
  const long long hw = (long long)h * w, feat_ns = (long long)nf * hw;
  SR_CHECK_ARG(hw * 4 * P.cin_pad0 < (1ll << 31), "%s: image too large for 32-bit plane offsets", who);
  SR_CHECK_ARG(((uintptr_t)d->packed_dgrad & 255u) == 0 && ((uintptr_t)d->workspace & 255u) == 0 && ((uintptr_t)d->stack & 255u) == 0,
               "%s: packed_dgrad, the stack and the workspace must be 256-byte aligned", who);
  SR_CHECK_ARG(sr::aligned16(d->in) && sr::aligned16(d->out) && sr::aligned16(d->dout) && sr::aligned16(d->din),
               "%s: in / out / dout / din must be 16-byte aligned", who);
  SR_CHECK_ARG(d->in_img_stride % 4 == 0 && d->dout_img_stride % 4 == 0 && (!d->din || d->din_img_stride % 4 == 0) &&
                   (nb > 0 || d->out_img_stride % 4 == 0),
               "%s: image strides must be multiples of 4 floats", who);
  SR_CHECK_ARG(n == 1 || (d->in_img_stride >= (long long)P.cin_pad0 * hw && d->dout_img_stride >= feat_ns &&
                          (!d->din || d->din_img_stride >= (long long)P.cin_pad0 * hw) && (nb > 0 || d->out_img_stride >= feat_ns)),
               "%s: an image stride is smaller than the image", who);
  SR_CHECK_ARG(nb > 0 || d->out != nullptr, "%s: num_block = 0 needs out, the LeakyReLU mask", who);
  SR_CHECK_ARG(d->din != d->in && d->din != d->dout, "%s: din must not be in or dout", who);
  const size_t one = sr::vsr_trunk_act_bytes(cfg, n, h, w), slab_bytes = sr_conv3x3_wgrad_slab_bytes(n, h, w);
  const size_t need = 3 * one + sr::align_up(slab_bytes, 256), stack_need = 2 * (size_t)nb * one;
  if (d->workspace_bytes < need) {
    sr::set_error("%s: workspace of %zu bytes, %zu needed (sr_vsr_trunk_bwd_workspace_bytes)", who, d->workspace_bytes, need);
    return SR_ENOSPACE;
  }
  if (stack_need > 0 && (!d->stack || d->stack_bytes < stack_need)) {
    sr::set_error("%s: stack of %zu bytes, %zu needed (sr_vsr_trunk_keep_bytes)", who, d->stack_bytes, stack_need);
    return SR_ENOSPACE;
  }
  for (size_t i = 0; i < P.convs.size(); ++i) {
    SR_CHECK_ARG(!d->dparams[2 * i + 1] || d->dparams[2 * i], "%s: the bias target of conv %zu needs its weight target", who, i);
    SR_CHECK_ARG(((uintptr_t)d->dparams[2 * i] & 3u) == 0 && ((uintptr_t)d->dparams[2 * i + 1] & 3u) == 0,
                 "%s: targets must be 4-byte aligned", who);
  }
  char* const ws = (char*)d->workspace;
  float* const gbuf[2] = {(float*)ws, (float*)(ws + one)};
  float* const dt = (float*)(ws + 2 * one);
  void* const slab = ws + 3 * one;
  const char* const packed = (const char*)d->packed_dgrad;
  auto act = [&](int i) -> const float* { return (const float*)((const char*)d->stack + (size_t)i * one); };

  // weight gradient of conv `ci` from its source and the gradient of its pre-activation output
  auto wgrad = [&](int ci, const float* x, long long x_ns, const float* dy, long long dy_ns) -> int {
    float* const dw = d->dparams[2 * ci];
    if (!dw) return SR_OK;
    const DgradConv& cp = P.convs[ci];
    sr_conv3x3_wgrad_desc q = {};
    q.x = x;
    q.x_img_stride = x_ns;
    q.cin_pad = cp.cin_pad;
    q.in_h = h;
    q.in_w = w;
    q.dy = dy;
    q.dy_img_stride = dy_ns;
    q.cout = cp.cout;
    q.cin = cp.cin;
    q.first_seg = cp.first_seg;
    q.seg = cp.seg;
    q.n = n;
    q.scale = 1.f;
    q.dweight = dw;
    q.dbias = d->dparams[2 * ci + 1];
    q.accumulate = d->accumulate;
    q.slab = slab;
    q.slab_bytes = slab_bytes;
    return sr_conv3x3_wgrad_f32(&q, stream);
  };
  // data gradient of conv `ci`: dx = conv(dy, mode-1 image) [+ res1] [masked]
  auto dgrad = [&](int ci, const float* dy, long long dy_ns, float* dx, long long dx_ns, const float* res1, long long res1_ns,
                   const float* mask, float slope) -> int {
    const DgradConv& cp = P.convs[ci];
    sr_conv3x3_desc q = {};
    q.in = dy;
    q.in_img_stride = dy_ns;
    q.cin_pad = cp.cout;
    q.cin_real = cp.cout;
    q.in_h = h;
    q.in_w = w;
    q.wpacked = (const float*)(packed + cp.w_off);
    q.cout = cp.cin_pad;
    q.out = dx;
    q.out_img_stride = dx_ns;
    q.n = n;
    q.act_slope = 1.f;
    q.alpha = 1.f;
    if (res1) {
      q.res1 = res1;
      q.res1_img_stride = res1_ns;
      q.beta1 = 1.f;
    }
    if (mask) {
      q.mask_src = mask;
      q.mask_img_stride = feat_ns;
      q.mask_cb0 = 0;
      q.mask_cbn = fb;
      q.mask_slope = slope;
    }
    return sr_conv3x3_f32(&q, stream);
  };

  const float* g = d->dout;
  long long g_ns = d->dout_img_stride;
  int cur = 0, rc = SR_OK;
  for (int b = nb - 1; b >= 0 && rc == SR_OK; --b) {
    const float *x = act(2 * b), *t = act(2 * b + 1);
    const int c1 = 1 + 2 * b, c2 = 2 + 2 * b;
    if ((rc = wgrad(c2, t, feat_ns, g, g_ns))) break;
    if ((rc = dgrad(c2, g, g_ns, dt, feat_ns, nullptr, 0, t, 0.f))) break;  // d(conv1 pre-activation)
    if ((rc = wgrad(c1, x, feat_ns, dt, feat_ns))) break;
    // d(block input) = conv1's data gradient + the identity path; block 0's input is the LeakyReLU output of the first conv
    if ((rc = dgrad(c1, dt, feat_ns, gbuf[cur], feat_ns, g, g_ns, b == 0 ? act(0) : nullptr, 0.1f))) break;
    g = gbuf[cur];
    g_ns = feat_ns;
    cur ^= 1;
  }
  if (rc) return rc;
  if (nb == 0) {
    rc = sr_cb8_relu_mask_f32(g, g_ns, d->out, d->out_img_stride, 0.1f, gbuf[0], feat_ns, n, fb, h, w, stream);
    if (rc) return rc;
    g = gbuf[0];
    g_ns = feat_ns;
  }
  if ((rc = wgrad(0, d->in, d->in_img_stride, g, g_ns))) return rc;
  if (!d->din) return SR_OK;
  return dgrad(0, g, g_ns, d->din, d->din_img_stride, nullptr, 0, nullptr, 0.f);
}
