// The recurrent video networks on gfx950 (include/sr_hip_vsr.h): the input of one propagation step, and the trunk driver.
//
// Reference: a step of BasicVSR / IconVSR (basicsr/archs/basicvsr_arch.py:62-68, :73-80) runs flow.permute, flow_warp, torch.cat
// and a ConvResidualBlocks of 1 + 2 * num_block convs on ONE low-resolution frame.  Here the step is one launch that writes the
// frame block and the warped feature where the first conv reads them (vsr_prop_input_kernel) and one C call that issues the convs
// (sr_vsr_trunk_f32), so that the per-launch cost of the step is that of the HIP runtime, not of a Python wrapper.
//
// vsr_prop_input_kernel is bandwidth-bound: per pixel and channel block four 32-byte corner reads and one 32-byte store.  A
// thread is one pixel of one block, consecutive lanes are consecutive pixels of a row, so a wave stores 2 KiB of consecutive
// addresses and the corner reads of neighbouring lanes share lines (a smooth flow moves neighbours together).  Blocks are
// blockIdx.y: with one thread per pixel alone a 180 x 320 frame would be 225 workgroups for 256 CUs, and each thread would hold
// four corners of every block at once.  The sampling position is recomputed per block: two loads and a dozen VALU operations.
#include <math.h>

#include <vector>

#include "../../include/sr_hip_vsr.h"
#include "sr_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// ---------------------------------------------------------------------------------------------- propagation step input
// The zeros-padding warp of flow_ops.hip (warp_coord, corners, blend), restated: position in fp32 with one rounding, floor and exact
// fraction, false where every corner lies outside the image.
__device__ __forceinline__ bool warp_coord_zeros(float flx, float fly, int x, int y, int H, int W, int& x0, int& y0, float& fx,
                                                 float& fy) {
  const float ix = W > 1 ? (float)x + flx : 0.f, iy = H > 1 ? (float)y + fly : 0.f;
  if (!(ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H)) return false;
  const float flx0 = floorf(ix), fly0 = floorf(iy);
  x0 = (int)flx0;
  y0 = (int)fly0;
  fx = ix - flx0;
  fy = iy - fly0;
  return true;
}
__device__ __forceinline__ float blend(double v00, double v01, double v10, double v11, float fx, float fy) {
  const double gx = fx, gy = fy;
  return (float)((1.0 - gy) * ((1.0 - gx) * v00 + gx * v01) + gy * ((1.0 - gx) * v10 + gx * v11));
}

struct PropParams {
  const float* frame;
  const float* prev;
  const float* flow;
  float* frame_out;
  float* warp_out;
  long long frame_ns, prev_ns, flow_ns, frame_out_ns, warp_out_ns;
  int H, W, fb;
};

// grid (ceil(HW / 256), fb [+ 1 with frame_out], n): blockIdx.y < fb warps one channel block, blockIdx.y == fb writes the frame block
__global__ __launch_bounds__(256) void vsr_prop_input_kernel(const PropParams p) {
  const int HW = p.H * p.W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int cb = blockIdx.y, n = blockIdx.z;
  if (cb == p.fb) {
    const float* f = p.frame + (long long)n * p.frame_ns + pix;
    float* dst = p.frame_out + (long long)n * p.frame_out_ns + (long long)pix * 8;
    *(f32x4*)dst = f32x4{f[0], f[HW], f[2 * (long long)HW], 0.f};
    *(f32x4*)(dst + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  float* dst = p.warp_out + (long long)n * p.warp_out_ns + ((long long)cb * HW + pix) * 8;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  if (p.prev) {
    const int py = pix / p.W, px = pix - py * p.W;
    const float* fl = p.flow + (long long)n * p.flow_ns + pix;
    int x0, y0;
    float fx, fy;
    if (warp_coord_zeros(fl[0], fl[HW], px, py, p.H, p.W, x0, y0, fx, fy)) {
      const bool xa = x0 >= 0 && x0 < p.W, xb = x0 + 1 >= 0 && x0 + 1 < p.W, ya = y0 >= 0 && y0 < p.H, yb = y0 + 1 >= 0 && y0 + 1 < p.H;
      const bool ok[4] = {ya && xa, ya && xb, yb && xa, yb && xb};
      const int o00 = y0 * p.W + x0;
      const int off[4] = {o00, o00 + 1, o00 + p.W, o00 + p.W + 1};
      const float* src = p.prev + (long long)n * p.prev_ns + (long long)cb * HW * 8;
      float v[4][8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
        if (ok[q]) {
          a = *(const f32x4*)(src + (long long)off[q] * 8);
          b = *(const f32x4*)(src + (long long)off[q] * 8 + 4);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[q][e] = a[e];
          v[q][4 + e] = b[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = blend(v[0][e], v[1][e], v[2][e], v[3][e], fx, fy);
    }
  }
  *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
  *(f32x4*)(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ---------------------------------------------------------------------------------------------------------- trunk plan
struct TrunkConv {
  int cout, cin, first_seg, seg, cin_pad;
  size_t w_off, b_off, wino_off;  // float offsets in the blob; kNoWino: the conv has no Winograd image
};
constexpr size_t kNoWino = ~(size_t)0;

struct TrunkPlan {
  std::vector<TrunkConv> convs;  // state_dict order
  size_t packed_floats, pack_entries;
  int cin_pad0;
};

bool make_plan(const sr_vsr_trunk_cfg* c, TrunkPlan* P) {
  if (!c || c->num_feat <= 0 || c->num_feat % 8 != 0 || c->num_feat > 4096 || c->num_block < 0 || c->num_block > 4096 ||
      (c->cin_segs != 1 && c->cin_segs != 2))
    return false;
  size_t off = 0;
  auto add = [&](int cout, int cin, int first_seg, int seg) {
    TrunkConv cp;
    cp.cout = cout;
    cp.cin = cin;
    cp.first_seg = first_seg;
    cp.seg = seg;
    cp.cin_pad = sr_conv3x3_cin_pad(cin, first_seg, seg);
    cp.w_off = off;
    off += sr::align_up(sr_conv3x3_packed_weight_floats(cout, cp.cin_pad), 64);
    cp.b_off = off;
    off += sr::align_up(sr_conv3x3_packed_bias_floats(cout), 64);
    cp.wino_off = kNoWino;
    P->convs.push_back(cp);
  };
  const int nf = c->num_feat;
  add(nf, 3 + c->cin_segs * nf, 3, nf);  // main.0
  for (int b = 0; b < c->num_block; ++b) {
    add(nf, nf, nf, 0);  // main.2.{b}.conv1
    add(nf, nf, nf, 0);  // main.2.{b}.conv2
  }
  P->cin_pad0 = P->convs[0].cin_pad;
  if (P->cin_pad0 != 8 + c->cin_segs * nf) return false;
  // Winograd F(2x2,3x3) images behind the direct images, whose offsets stay (as rrdbnet.hip)
  P->pack_entries = P->convs.size();
  for (TrunkConv& cp : P->convs) {
    if (!sr::wino_f32_weights_eligible(cp.cout, cp.cin)) continue;
    cp.wino_off = off;
    off += sr::align_up(sr::wino_f32_image_floats(cp.cout, cp.cin_pad), 64);
    ++P->pack_entries;
  }
  P->packed_floats = off;
  return true;
}

size_t act_bytes(int nf, int n, int h, int w) { return sr::align_up((size_t)n * nf * h * w * sizeof(float), 256); }

}  // namespace

extern "C" int sr_vsr_prop_input_f32(const sr_vsr_prop_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_vsr_prop_input_f32: null descriptor");
  SR_CHECK_ARG(d->frame && d->warp_out, "sr_vsr_prop_input_f32: null frame / warp_out");
  SR_CHECK_ARG((d->prev == nullptr) == (d->flow == nullptr), "sr_vsr_prop_input_f32: prev and flow must both be given or both be NULL");
  SR_CHECK_ARG(d->n > 0 && d->n <= 65535 && d->h > 0 && d->w > 0 && d->fb > 0 && d->fb < 65535,
               "sr_vsr_prop_input_f32: bad shape n=%d h=%d w=%d fb=%d", d->n, d->h, d->w, d->fb);
  const long long hw = (long long)d->h * d->w;
  SR_CHECK_ARG(hw < (1ll << 28), "sr_vsr_prop_input_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(aligned16(d->prev) && aligned16(d->frame_out) && aligned16(d->warp_out),
               "sr_vsr_prop_input_f32: CB8 windows must be 16-byte aligned");
  SR_CHECK_ARG(((uintptr_t)d->frame & 3u) == 0 && ((uintptr_t)d->flow & 3u) == 0, "sr_vsr_prop_input_f32: frame / flow must be 4-byte aligned");
  SR_CHECK_ARG(d->prev_img_stride % 4 == 0 && d->frame_out_img_stride % 4 == 0 && d->warp_out_img_stride % 4 == 0,
               "sr_vsr_prop_input_f32: image strides of CB8 windows must be multiples of 4 floats");
  SR_CHECK_ARG(d->n == 1 || (d->frame_img_stride >= 3 * hw && d->warp_out_img_stride >= hw * 8 * d->fb &&
                             (!d->prev || (d->prev_img_stride >= hw * 8 * d->fb && d->flow_img_stride >= 2 * hw)) &&
                             (!d->frame_out || d->frame_out_img_stride >= hw * 8)),
               "sr_vsr_prop_input_f32: an image stride is smaller than the image");
  PropParams p = {};
  p.frame = d->frame;
  p.prev = d->prev;
  p.flow = d->flow;
  p.frame_out = d->frame_out;
  p.warp_out = d->warp_out;
  p.frame_ns = d->frame_img_stride;
  p.prev_ns = d->prev_img_stride;
  p.flow_ns = d->flow_img_stride;
  p.frame_out_ns = d->frame_out_img_stride;
  p.warp_out_ns = d->warp_out_img_stride;
  p.H = d->h;
  p.W = d->w;
  p.fb = d->fb;
  const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)(d->fb + (d->frame_out ? 1 : 0)), (unsigned)d->n);
  const bool prof = sr::prof_on();
  if (prof) {
    sr_launch_record r = {};
    r.kernel_id = 159;
    r.cin = r.cout = 8 * d->fb;
    r.n = d->n;
    r.h = d->h;
    r.w = d->w;
    const double px = (double)d->n * (double)hw;
    r.flops = d->prev ? 8.0 * 8.0 * d->fb * px : 0.0;
    r.bytes = 4.0 * px * ((d->prev ? 5.0 : 1.0) * 8.0 * d->fb + (d->prev ? 2.0 * d->fb : 0.0) + (d->frame_out ? 11.0 : 0.0));
    sr::prof_begin(stream, r);
  }
  hipLaunchKernelGGL(vsr_prop_input_kernel, grid, dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_vsr_prop_input_f32 launch");
  return SR_OK;
}

extern "C" int sr_vsr_trunk_num_params(const sr_vsr_trunk_cfg* cfg) {
  TrunkPlan P;
  SR_CHECK_ARG(make_plan(cfg, &P), "sr_vsr_trunk_num_params: bad config (num_feat a multiple of 8, num_block >= 0, cin_segs 1 or 2)");
  return 2 * (int)P.convs.size();
}

extern "C" int sr_vsr_trunk_conv_wino(const sr_vsr_trunk_cfg* cfg, int index) {
  TrunkPlan P;
  SR_CHECK_ARG(make_plan(cfg, &P), "sr_vsr_trunk_conv_wino: bad config (num_feat a multiple of 8, num_block >= 0, cin_segs 1 or 2)");
  SR_CHECK_ARG(index >= 0 && (size_t)index < P.convs.size(), "sr_vsr_trunk_conv_wino: conv %d of %zu", index, P.convs.size());
  return P.convs[index].wino_off != kNoWino ? 1 : 0;
}

extern "C" size_t sr_vsr_trunk_packed_bytes(const sr_vsr_trunk_cfg* cfg) {
  TrunkPlan P;
  if (!make_plan(cfg, &P)) return 0;
  return P.packed_floats * sizeof(float) + sr::pack_table_bytes(P.pack_entries);
}

extern "C" size_t sr_vsr_trunk_workspace_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w) {
  TrunkPlan P;
  if (!make_plan(cfg, &P) || n <= 0 || h <= 0 || w <= 0) return 0;
  return 3 * act_bytes(cfg->num_feat, n, h, w);
}

extern "C" int sr_vsr_trunk_pack_f32(const sr_vsr_trunk_cfg* cfg, const float* const* params, float* packed, void* stream) {
  TrunkPlan P;
  SR_CHECK_ARG(make_plan(cfg, &P), "sr_vsr_trunk_pack_f32: bad config (num_feat a multiple of 8, num_block >= 0, cin_segs 1 or 2)");
  SR_CHECK_ARG(params && packed, "sr_vsr_trunk_pack_f32: null argument");
  SR_CHECK_ARG(((uintptr_t)packed & 255u) == 0, "sr_vsr_trunk_pack_f32: packed must be 256-byte aligned");
  std::vector<sr::PackEntry> tab(P.convs.size());  // one launch for all images (pack_net.hip)
  for (size_t i = 0; i < P.convs.size(); ++i) {
    const TrunkConv& cp = P.convs[i];
    SR_CHECK_ARG(params[2 * i] && params[2 * i + 1], "sr_vsr_trunk_pack_f32: null parameter %zu", i);
    sr::PackEntry& e = tab[i];
    e = sr::PackEntry{};
    e.kind = 0;
    e.w[0] = params[2 * i];
    e.bias = params[2 * i + 1];
    e.out = packed + cp.w_off;
    e.bout = packed + cp.b_off;
    e.cout = cp.cout;
    e.cin = cp.cin;
    e.first_seg = cp.first_seg;
    e.seg = cp.seg > 0 ? cp.seg : 1;
    e.cin_pad = cp.cin_pad;
  }
  for (size_t i = 0; i < P.convs.size(); ++i) {  // the Winograd images of the same weights
    const TrunkConv& cp = P.convs[i];
    if (cp.wino_off == kNoWino) continue;
    sr::PackEntry e = tab[i];
    e.kind = 3;
    e.bias = nullptr;
    e.bout = nullptr;
    e.out = packed + cp.wino_off;
    tab.push_back(e);
  }
  return sr::pack_table_run(tab, packed, P.packed_floats * sizeof(float), false, (hipStream_t)stream);
}

extern "C" int sr_vsr_trunk_f32(const sr_vsr_trunk_cfg* cfg, const float* packed, const float* in, long long in_img_stride, float* out,
                                long long out_img_stride, int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TrunkPlan P;
  SR_CHECK_ARG(make_plan(cfg, &P), "sr_vsr_trunk_f32: bad config (num_feat a multiple of 8, num_block >= 0, cin_segs 1 or 2)");
  SR_CHECK_ARG(packed && in && out, "sr_vsr_trunk_f32: null packed / in / out");
  SR_CHECK_ARG(n > 0 && h > 0 && w > 0, "sr_vsr_trunk_f32: bad shape n=%d h=%d w=%d", n, h, w);
  const int nf = cfg->num_feat;
  const long long hw = (long long)h * w, feat_ns = (long long)nf * hw;
  SR_CHECK_ARG(hw * 4 * P.cin_pad0 < (1ll << 31), "sr_vsr_trunk_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(aligned16(packed) && aligned16(in) && aligned16(out) && ((uintptr_t)workspace & 255u) == 0,
               "sr_vsr_trunk_f32: packed / in / out must be 16-byte, the workspace 256-byte aligned");
  SR_CHECK_ARG(in_img_stride % 4 == 0 && out_img_stride % 4 == 0, "sr_vsr_trunk_f32: image strides must be multiples of 4 floats");
  SR_CHECK_ARG(n == 1 || (in_img_stride >= (long long)P.cin_pad0 * hw && out_img_stride >= feat_ns),
               "sr_vsr_trunk_f32: an image stride is smaller than the image");
  const size_t need = cfg->num_block > 0 ? 3 * act_bytes(nf, n, h, w) : 0;
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    sr::set_error("sr_vsr_trunk_f32: workspace of %zu bytes, %zu needed (sr_vsr_trunk_workspace_bytes)", workspace_bytes, need);
    return SR_ENOSPACE;
  }
  float* buf[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3 && need; ++i) buf[i] = (float*)((char*)workspace + (size_t)i * act_bytes(nf, n, h, w));

  const bool wino = sr::wino_f32_mode() != 0;
  size_t ci = 0;
  auto conv = [&](const float* src, long long src_ns, float* dst, long long dst_ns, float slope, const float* res1) -> int {
    const TrunkConv& cp = P.convs[ci++];
    sr_conv3x3_desc d = {};
    d.in = src;
    d.in_img_stride = src_ns;
    d.cin_pad = cp.cin_pad;
    d.cin_real = cp.cin;
    d.in_h = h;
    d.in_w = w;
    d.wpacked = packed + cp.w_off;
    d.bpacked = packed + cp.b_off;
    d.cout = cp.cout;
    d.out = dst;
    d.out_img_stride = dst_ns;
    d.n = n;
    d.act_slope = slope;
    d.alpha = 1.f;
    if (res1) {
      d.res1 = res1;
      d.res1_img_stride = feat_ns;
      d.beta1 = 1.f;
    }
    if (wino && cp.wino_off != kNoWino) {
      const int rc = sr::conv3x3_wino_f32(&d, packed + cp.wino_off, stream, false);
      if (rc != SR_WINO_NOT_ELIGIBLE) return rc;
    }
    return sr_conv3x3_f32(&d, stream);
  };

  const int nb = cfg->num_block;
  // main.0 + LeakyReLU(0.1)
  int rc = nb == 0 ? conv(in, in_img_stride, out, out_img_stride, 0.1f, nullptr) : conv(in, in_img_stride, buf[0], feat_ns, 0.1f, nullptr);
  int x = 0;  // buffer that holds the block input
  for (int b = 0; b < nb && rc == SR_OK; ++b) {
    const int t = (x + 1) % 3, y = (x + 2) % 3;
    rc = conv(buf[x], feat_ns, buf[t], feat_ns, 0.f, nullptr);  // relu(conv1(x))
    if (rc) break;
    if (b + 1 == nb)
      rc = conv(buf[t], feat_ns, out, out_img_stride, 1.f, buf[x]);  // x + conv2(.)
    else
      rc = conv(buf[t], feat_ns, buf[y], feat_ns, 1.f, buf[x]);
    x = y;
  }
  return rc;
}
