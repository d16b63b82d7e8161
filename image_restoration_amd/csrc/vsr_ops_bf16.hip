// The recurrent video networks in bf16 on gfx950 (include/sr_hip_vsr_bf16.h): the input of one propagation step on CB16, and the
// trunk driver on sr_conv3x3_bf16.  The CB16 twins of vsr_ops.hip.
//
// vsr_prop_input_bf16_kernel is bandwidth-bound like its fp32 twin: per pixel and channel block four 32-byte corner reads and one
// 32-byte store, now for 16 channels.  A thread is one pixel of one block, consecutive lanes are consecutive pixels of a row, and a
// thread moves whole 16-byte pieces: the 32-byte pixel is two b128 loads per corner and two b128 stores, done half by half so that
// only eight channels' corners are widened at once.  Blocks are blockIdx.y, so a 180 x 320 frame of 64 channels is 225 x 4 (+ 1)
// workgroups for 256 CUs.  The flow stays fp32 and the sampling position is recomputed per block, as in fp32.  No LDS, no atomics.
//
// The arithmetic is fixed (the header): corners widened to fp32, the fp32 kernel's position / floor / fraction / corner rule, the
// float64 blend rounded once to fp32, then one round-to-nearest-even to bf16.
#include <math.h>

#include <vector>

#include "../../include/sr_hip_vsr_bf16.h"
#include "sr_internal.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

// ---------------------------------------------------------------------------------------------- propagation step input
// warp_coord_zeros and blend are those of vsr_ops.hip, restated (both live in anonymous namespaces).
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
// bf16 <-> fp32 on the bit patterns: widening is exact, narrowing rounds to nearest even
__device__ __forceinline__ float widen_lo(unsigned int pair) { return __uint_as_float(pair << 16); }
__device__ __forceinline__ float widen_hi(unsigned int pair) { return __uint_as_float(pair & 0xffff0000u); }
__device__ __forceinline__ unsigned int narrow(float v) { return (unsigned int)__builtin_bit_cast(unsigned short, (__bf16)v); }
__device__ __forceinline__ unsigned int narrow2(float lo, float hi) { return narrow(lo) | (narrow(hi) << 16); }

struct PropParamsH {
  const float* frame;
  const unsigned short* prev;
  const float* flow;
  unsigned short* frame_out;
  unsigned short* warp_out;
  long long frame_ns, prev_ns, flow_ns, frame_out_ns, warp_out_ns;
  int H, W, fb;
};

// grid (ceil(HW / 256), fb [+ 1 with frame_out], n): blockIdx.y < fb warps one channel block, blockIdx.y == fb writes the frame block
__global__ __launch_bounds__(256) void vsr_prop_input_bf16_kernel(const PropParamsH p) {
  const int HW = p.H * p.W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int cb = blockIdx.y, n = blockIdx.z;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  if (cb == p.fb) {
    const float* f = p.frame + (long long)n * p.frame_ns + pix;
    unsigned short* dst = p.frame_out + (long long)n * p.frame_out_ns + (long long)pix * 16;
    *(u32x4*)dst = u32x4{narrow2(f[0], f[HW]), narrow(f[2 * (long long)HW]), 0u, 0u};
    *(u32x4*)(dst + 8) = zero;
    return;
  }
  unsigned short* dst = p.warp_out + (long long)n * p.warp_out_ns + ((long long)cb * HW + pix) * 16;
  u32x4 o[2] = {zero, zero};
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
      const unsigned short* src = p.prev + (long long)n * p.prev_ns + (long long)cb * HW * 16;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        u32x4 c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          c[q] = zero;
          if (ok[q]) c[q] = *(const u32x4*)(src + (long long)off[q] * 16 + half * 8);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = blend(widen_lo(c[0][e]), widen_lo(c[1][e]), widen_lo(c[2][e]), widen_lo(c[3][e]), fx, fy);
          const float hi = blend(widen_hi(c[0][e]), widen_hi(c[1][e]), widen_hi(c[2][e]), widen_hi(c[3][e]), fx, fy);
          o[half][e] = narrow2(lo, hi);
        }
      }
    }
  }
  *(u32x4*)dst = o[0];
  *(u32x4*)(dst + 8) = o[1];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ---------------------------------------------------------------------------------------------------------- trunk plan
struct TrunkConvH {
  int cout, cin, first_seg, seg, cin_pad;
  size_t w_off, b_off;  // byte offsets in the blob
};

struct TrunkPlanH {
  std::vector<TrunkConvH> convs;  // state_dict order
  size_t packed_bytes;
  int cin_pad0;
};

bool make_plan_h(const sr_vsr_trunk_cfg* c, TrunkPlanH* P) {
  if (!c || c->num_feat <= 0 || c->num_feat % 16 != 0 || c->num_feat > 4096 || c->num_block < 0 || c->num_block > 4096 ||
      (c->cin_segs != 1 && c->cin_segs != 2))
    return false;
  size_t off = 0;
  auto add = [&](int cout, int cin, int first_seg, int seg) {
    TrunkConvH cp;
    cp.cout = cout;
    cp.cin = cin;
    cp.first_seg = first_seg;
    cp.seg = seg;
    cp.cin_pad = sr_conv3x3_cin_pad16(cin, first_seg, seg);
    cp.w_off = off;
    off += sr::align_up(sr_conv3x3_packed_weight_elems_bf16(cout, cin, first_seg, seg, 0) * 2, 256);
    cp.b_off = off;
    off += sr::align_up(sr_conv3x3_packed_bias_floats(cout) * 4, 256);
    P->convs.push_back(cp);
  };
  const int nf = c->num_feat;
  add(nf, 3 + c->cin_segs * nf, 3, nf);  // main.0
  for (int b = 0; b < c->num_block; ++b) {
    add(nf, nf, nf, 0);  // main.2.{b}.conv1
    add(nf, nf, nf, 0);  // main.2.{b}.conv2
  }
  P->cin_pad0 = P->convs[0].cin_pad;
  if (P->cin_pad0 != 16 + c->cin_segs * nf) return false;
  P->packed_bytes = off;
  return true;
}

size_t act_bytes_h(int nf, int n, int h, int w) { return sr::align_up((size_t)n * nf * h * w * 2, 256); }

#define RVSR_BAD_CFG "bad config (num_feat a multiple of 16, num_block >= 0, cin_segs 1 or 2)"

}  // namespace

extern "C" int sr_rvsr_prop_input_bf16(const sr_rvsr_prop_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_rvsr_prop_input_bf16: null descriptor");
  SR_CHECK_ARG(d->frame && d->warp_out, "sr_rvsr_prop_input_bf16: null frame / warp_out");
  SR_CHECK_ARG((d->prev == nullptr) == (d->flow == nullptr), "sr_rvsr_prop_input_bf16: prev and flow must both be given or both be NULL");
  SR_CHECK_ARG(d->n > 0 && d->n <= 65535 && d->h > 0 && d->w > 0 && d->fb > 0 && d->fb < 65535,
               "sr_rvsr_prop_input_bf16: bad shape n=%d h=%d w=%d fb=%d", d->n, d->h, d->w, d->fb);
  const long long hw = (long long)d->h * d->w;
  SR_CHECK_ARG(hw < (1ll << 28), "sr_rvsr_prop_input_bf16: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(aligned16(d->prev) && aligned16(d->frame_out) && aligned16(d->warp_out),
               "sr_rvsr_prop_input_bf16: CB16 windows must be 16-byte aligned");
  SR_CHECK_ARG(((uintptr_t)d->frame & 3u) == 0 && ((uintptr_t)d->flow & 3u) == 0, "sr_rvsr_prop_input_bf16: frame / flow must be 4-byte aligned");
  SR_CHECK_ARG(d->prev_img_stride % 8 == 0 && d->frame_out_img_stride % 8 == 0 && d->warp_out_img_stride % 8 == 0,
               "sr_rvsr_prop_input_bf16: image strides of CB16 windows must be multiples of 8 elements");
  SR_CHECK_ARG(d->n == 1 || (d->frame_img_stride >= 3 * hw && d->warp_out_img_stride >= hw * 16 * d->fb &&
                             (!d->prev || (d->prev_img_stride >= hw * 16 * d->fb && d->flow_img_stride >= 2 * hw)) &&
                             (!d->frame_out || d->frame_out_img_stride >= hw * 16)),
               "sr_rvsr_prop_input_bf16: an image stride is smaller than the image");
  PropParamsH p = {};
  p.frame = d->frame;
  p.prev = (const unsigned short*)d->prev;
  p.flow = d->flow;
  p.frame_out = (unsigned short*)d->frame_out;
  p.warp_out = (unsigned short*)d->warp_out;
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
    r.kernel_id = 167;
    r.cin = r.cout = 16 * d->fb;
    r.n = d->n;
    r.h = d->h;
    r.w = d->w;
    const double px = (double)d->n * (double)hw;
    // per pixel and block: 16 channels x 8 flops; four 32-byte corners and one 32-byte store, the two fp32 flow values; the frame
    // block reads 12 and writes 32 bytes
    r.flops = d->prev ? 8.0 * 16.0 * d->fb * px : 0.0;
    r.bytes = px * ((d->prev ? 5.0 : 1.0) * 32.0 * d->fb + (d->prev ? 8.0 * d->fb : 0.0) + (d->frame_out ? 44.0 : 0.0));
    sr::prof_begin(stream, r);
  }
  hipLaunchKernelGGL(vsr_prop_input_bf16_kernel, grid, dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_rvsr_prop_input_bf16 launch");
  return SR_OK;
}

extern "C" size_t sr_rvsr_trunk_packed_bytes_bf16(const sr_vsr_trunk_cfg* cfg) {
  TrunkPlanH P;
  if (!make_plan_h(cfg, &P)) return 0;
  return P.packed_bytes + sr::pack_table_bytes(P.convs.size());
}

extern "C" size_t sr_rvsr_trunk_workspace_bytes_bf16(const sr_vsr_trunk_cfg* cfg, int n, int h, int w) {
  TrunkPlanH P;
  if (!make_plan_h(cfg, &P) || n <= 0 || h <= 0 || w <= 0) return 0;
  return 3 * act_bytes_h(cfg->num_feat, n, h, w);
}

extern "C" int sr_rvsr_trunk_pack_bf16(const sr_vsr_trunk_cfg* cfg, const float* const* params, void* packed, void* stream) {
  TrunkPlanH P;
  SR_CHECK_ARG(make_plan_h(cfg, &P), "sr_rvsr_trunk_pack_bf16: " RVSR_BAD_CFG);
  SR_CHECK_ARG(params && packed, "sr_rvsr_trunk_pack_bf16: null argument");
  SR_CHECK_ARG(((uintptr_t)packed & 255u) == 0, "sr_rvsr_trunk_pack_bf16: packed must be 256-byte aligned");
  std::vector<sr::PackEntry> tab(P.convs.size());  // one launch for all images (pack_net.hip), as sr_rrdbnet_pack_bf16
  for (size_t i = 0; i < P.convs.size(); ++i) {
    const TrunkConvH& cp = P.convs[i];
    SR_CHECK_ARG(params[2 * i] && params[2 * i + 1], "sr_rvsr_trunk_pack_bf16: null parameter %zu", i);
    sr::PackEntry& e = tab[i];
    e = sr::PackEntry{};
    e.kind = 0;
    e.w[0] = params[2 * i];
    e.bias = params[2 * i + 1];
    e.out = (char*)packed + cp.w_off;
    e.bout = (float*)((char*)packed + cp.b_off);
    e.cout = cp.cout;
    e.cin = cp.cin;
    e.first_seg = cp.first_seg;
    e.seg = cp.seg > 0 ? cp.seg : 1;
    e.cin_pad = cp.cin_pad;
  }
  return sr::pack_table_run(tab, packed, P.packed_bytes, true, (hipStream_t)stream);
}

extern "C" int sr_rvsr_trunk_bf16(const sr_vsr_trunk_cfg* cfg, const void* packed, const void* in, long long in_img_stride, void* out,
                                  long long out_img_stride, int n, int h, int w, void* workspace, size_t workspace_bytes,
                                  void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TrunkPlanH P;
  SR_CHECK_ARG(make_plan_h(cfg, &P), "sr_rvsr_trunk_bf16: " RVSR_BAD_CFG);
  SR_CHECK_ARG(packed && in && out, "sr_rvsr_trunk_bf16: null packed / in / out");
  SR_CHECK_ARG(n > 0 && h > 0 && w > 0, "sr_rvsr_trunk_bf16: bad shape n=%d h=%d w=%d", n, h, w);
  const int nf = cfg->num_feat;
  const long long hw = (long long)h * w, feat_ns = (long long)nf * hw;
  SR_CHECK_ARG(hw * 2 * P.cin_pad0 < (1ll << 31), "sr_rvsr_trunk_bf16: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(aligned16(packed) && aligned16(in) && aligned16(out) && ((uintptr_t)workspace & 255u) == 0,
               "sr_rvsr_trunk_bf16: packed / in / out must be 16-byte, the workspace 256-byte aligned");
  SR_CHECK_ARG(in_img_stride % 8 == 0 && out_img_stride % 8 == 0, "sr_rvsr_trunk_bf16: image strides must be multiples of 8 elements");
  SR_CHECK_ARG(n == 1 || (in_img_stride >= (long long)P.cin_pad0 * hw && out_img_stride >= feat_ns),
               "sr_rvsr_trunk_bf16: an image stride is smaller than the image");
  const size_t one = act_bytes_h(nf, n, h, w), need = cfg->num_block > 0 ? 3 * one : 0;
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    sr::set_error("sr_rvsr_trunk_bf16: workspace of %zu bytes, %zu needed (sr_rvsr_trunk_workspace_bytes_bf16)", workspace_bytes, need);
    return SR_ENOSPACE;
  }
  void* buf[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3 && need; ++i) buf[i] = (char*)workspace + (size_t)i * one;

  size_t ci = 0;
  auto conv = [&](const void* src, long long src_ns, void* dst, long long dst_ns, float slope, const void* res1) -> int {
    const TrunkConvH& cp = P.convs[ci++];
    sr_conv3x3_desc d = {};
    d.in = (const float*)src;
    d.in_img_stride = src_ns;
    d.cin_pad = cp.cin_pad;
    d.cin_real = cp.cin;
    d.in_h = h;
    d.in_w = w;
    d.wpacked = (const float*)((const char*)packed + cp.w_off);
    d.bpacked = (const float*)((const char*)packed + cp.b_off);
    d.cout = cp.cout;
    d.out = (float*)dst;
    d.out_img_stride = dst_ns;
    d.n = n;
    d.act_slope = slope;
    d.alpha = 1.f;
    if (res1) {
      d.res1 = (const float*)res1;
      d.res1_img_stride = feat_ns;
      d.beta1 = 1.f;
    }
    return sr_conv3x3_bf16(&d, stream);
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
