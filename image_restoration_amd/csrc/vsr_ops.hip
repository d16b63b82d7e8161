// The recurrent video networks on gfx950, fp32 on CB8 (include/sr_hip_vsr.h) and bf16 on CB16 (include/sr_hip_vsr_bf16.h): the
// input of one propagation step, and the trunk driver.  One translation unit for both element types: the two step-input kernels
// differ (how a thread moves its pixel), everything on the host is written once and told apart by a Kind record.
//
// Reference: a step of BasicVSR / IconVSR (basicsr/archs/basicvsr_arch.py:62-68, :73-80) runs flow.permute, flow_warp, torch.cat
// and a ConvResidualBlocks of 1 + 2 * num_block convs on ONE low-resolution frame.  Here the step is one launch that writes the
// frame block and the warped feature where the first conv reads them (vsr_prop_input_kernel / vsr_prop_input_bf16_kernel) and one
// C call that issues the convs (sr_vsr_trunk_f32 / sr_rvsr_trunk_bf16), so that the per-launch cost of the step is that of the HIP
// runtime, not of a Python wrapper.
//
// The step-input kernels are bandwidth-bound: per pixel and channel block four 32-byte corner reads and one 32-byte store (8 fp32
// or 16 bf16 channels).  A thread is one pixel of one block, consecutive lanes are consecutive pixels of a row, so a wave stores
// 2 KiB of consecutive addresses and the corner reads of neighbouring lanes share lines (a smooth flow moves neighbours together).
// Blocks are blockIdx.y: with one thread per pixel alone a 180 x 320 frame would be 225 workgroups for 256 CUs, and each thread
// would hold four corners of every block at once.  The sampling position is recomputed per block: two loads and a dozen VALU
// operations.  The bf16 kernel moves whole 16-byte pieces: its 32-byte pixel is two b128 loads per corner and two b128 stores, done
// half by half so that only eight channels' corners are widened at once.  The flow stays fp32 in both.  No LDS, no atomics.
//
// The sampling position and the blend are flow_device.h's (zeros padding), shared with flow_ops.hip; the four corner tests stay
// written out in the kernels, since flowdev::corners makes the compiler swap the operands of one s_and_b64 in the fp32 kernel and
// the kernels are kept instruction for instruction.  The bf16 arithmetic is fixed (its header):
// corners widened to fp32, the fp32 kernel's position / floor / fraction / corner rule, the float64 blend rounded once to fp32,
// then one round-to-nearest-even to bf16.
#include <math.h>

#include <vector>

#include "../../include/sr_hip_vsr.h"
#include "../../include/sr_hip_vsr_bf16.h"
#include "flow_device.h"
#include "sr_internal.h"
#include "vsr_trunk.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

// ---------------------------------------------------------------------------------------------- propagation step input
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
    bool gx_on, gy_on;  // the backward's gradient switches, unused
    if (flowdev::warp_coord(fl[0], fl[HW], px, py, p.H, p.W, /*border=*/0, x0, y0, fx, fy, gx_on, gy_on)) {
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
      for (int e = 0; e < 8; ++e) o[e] = flowdev::blend(v[0][e], v[1][e], v[2][e], v[3][e], fx, fy);
    }
  }
  *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
  *(f32x4*)(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
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

// the same grid on CB16
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
    bool gx_on, gy_on;  // the backward's gradient switches, unused
    if (flowdev::warp_coord(fl[0], fl[HW], px, py, p.H, p.W, /*border=*/0, x0, y0, fx, fy, gx_on, gy_on)) {
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
          const float lo = flowdev::blend(widen_lo(c[0][e]), widen_lo(c[1][e]), widen_lo(c[2][e]), widen_lo(c[3][e]), fx, fy);
          const float hi = flowdev::blend(widen_hi(c[0][e]), widen_hi(c[1][e]), widen_hi(c[2][e]), widen_hi(c[3][e]), fx, fy);
          o[half][e] = narrow2(lo, hi);
        }
      }
    }
  }
  *(u32x4*)dst = o[0];
  *(u32x4*)(dst + 8) = o[1];
}

// What tells the two element types apart on the host: channels per block, element bytes, and the words of the messages.  A 16-byte
// piece is 16 / elem elements, which is the multiple every window stride must be.
struct Kind {
  bool bf16;
  int lanes, elem;
  const char *window, *unit;
};
constexpr Kind kF32 = {false, 8, 4, "CB8", "floats"}, kBf16 = {true, 16, 2, "CB16", "elements"};

// Checks, parameter struct, profiler record and launch of a step input; `who` is the entry point, Desc its descriptor (the two
// have the same fields), Params what `kernel` takes.
template <class Desc, class Params>
int prop_input(const Kind& k, const char* who, int kernel_id, void (*kernel)(Params), const Desc* d, hipStream_t stream) {
  SR_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  SR_CHECK_ARG(d->frame && d->warp_out, "%s: null frame / warp_out", who);
  SR_CHECK_ARG((d->prev == nullptr) == (d->flow == nullptr), "%s: prev and flow must both be given or both be NULL", who);
  SR_CHECK_ARG(d->n > 0 && d->n <= 65535 && d->h > 0 && d->w > 0 && d->fb > 0 && d->fb < 65535, "%s: bad shape n=%d h=%d w=%d fb=%d",
               who, d->n, d->h, d->w, d->fb);
  const long long hw = (long long)d->h * d->w, mult = 16 / k.elem, blk = hw * k.lanes;
  SR_CHECK_ARG(hw < (1ll << 28), "%s: image too large for 32-bit plane offsets", who);
  SR_CHECK_ARG(sr::aligned16(d->prev) && sr::aligned16(d->frame_out) && sr::aligned16(d->warp_out),
               "%s: %s windows must be 16-byte aligned", who, k.window);
  SR_CHECK_ARG(((uintptr_t)d->frame & 3u) == 0 && ((uintptr_t)d->flow & 3u) == 0, "%s: frame / flow must be 4-byte aligned", who);
  SR_CHECK_ARG(d->prev_img_stride % mult == 0 && d->frame_out_img_stride % mult == 0 && d->warp_out_img_stride % mult == 0,
               "%s: image strides of %s windows must be multiples of %lld %s", who, k.window, mult, k.unit);
  SR_CHECK_ARG(d->n == 1 || (d->frame_img_stride >= 3 * hw && d->warp_out_img_stride >= blk * d->fb &&
                             (!d->prev || (d->prev_img_stride >= blk * d->fb && d->flow_img_stride >= 2 * hw)) &&
                             (!d->frame_out || d->frame_out_img_stride >= blk)),
               "%s: an image stride is smaller than the image", who);
  Params p = {};
  p.frame = d->frame;
  p.prev = (decltype(p.prev))d->prev;
  p.flow = d->flow;
  p.frame_out = (decltype(p.frame_out))d->frame_out;
  p.warp_out = (decltype(p.warp_out))d->warp_out;
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
    r.kernel_id = kernel_id;
    r.cin = r.cout = k.lanes * d->fb;
    r.n = d->n;
    r.h = d->h;
    r.w = d->w;
    const double px = (double)d->n * (double)hw;
    // per pixel and block: 8 flops a channel; four 32-byte corners and one 32-byte store, the two fp32 flow values; the frame
    // block reads 12 and writes 32 bytes
    r.flops = d->prev ? 8.0 * k.lanes * d->fb * px : 0.0;
    r.bytes = px * ((d->prev ? 5.0 : 1.0) * 32.0 * d->fb + (d->prev ? 8.0 * d->fb : 0.0) + (d->frame_out ? 44.0 : 0.0));
    sr::prof_begin(stream, r);
  }
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    sr::set_error("%s launch: %s", who, hipGetErrorString(e));
    return SR_ELAUNCH;
  }
  return SR_OK;
}

// ---------------------------------------------------------------------------------------------------------- trunk plan
struct TrunkConv {
  int cout, cin, first_seg, seg, cin_pad;
  size_t w_off, b_off, wino_off;  // byte offsets in the blob, multiples of 256; kNoWino: the conv has no Winograd image
};
constexpr size_t kNoWino = ~(size_t)0;

struct TrunkPlan {
  std::vector<TrunkConv> convs;  // state_dict order
  size_t packed_bytes, pack_entries;
  int cin_pad0;
};

bool make_plan(const sr_vsr_trunk_cfg* c, const Kind& k, TrunkPlan* P) {
  if (!c || c->num_feat <= 0 || c->num_feat % k.lanes != 0 || c->num_feat > 4096 || c->num_block < 0 || c->num_block > 4096 ||
      (c->cin_segs != 1 && c->cin_segs != 2))
    return false;
  size_t off = 0;
  auto add = [&](int cout, int cin, int first_seg, int seg) {
    TrunkConv cp;
    cp.cout = cout;
    cp.cin = cin;
    cp.first_seg = first_seg;
    cp.seg = seg;
    cp.cin_pad = k.bf16 ? sr_conv3x3_cin_pad16(cin, first_seg, seg) : sr_conv3x3_cin_pad(cin, first_seg, seg);
    cp.w_off = off;
    off += sr::align_up(k.bf16 ? sr_conv3x3_packed_weight_elems_bf16(cout, cin, first_seg, seg, 0) * 2
                               : sr_conv3x3_packed_weight_floats(cout, cp.cin_pad) * 4,
                        256);
    cp.b_off = off;
    off += sr::align_up(sr_conv3x3_packed_bias_floats(cout) * 4, 256);
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
  if (P->cin_pad0 != k.lanes + c->cin_segs * nf) return false;
  // fp32: Winograd F(2x2,3x3) images behind the direct images, whose offsets stay (as rrdbnet.hip)
  P->pack_entries = P->convs.size();
  for (TrunkConv& cp : P->convs) {
    if (k.bf16 || !sr::wino_f32_weights_eligible(cp.cout, cp.cin)) continue;
    cp.wino_off = off;
    off += sr::align_up(sr::wino_f32_image_floats(cp.cout, cp.cin_pad) * 4, 256);
    ++P->pack_entries;
  }
  P->packed_bytes = off;
  return true;
}

size_t act_bytes(const Kind& k, int nf, int n, int h, int w) { return sr::align_up((size_t)n * nf * h * w * k.elem, 256); }

size_t trunk_packed_bytes(const sr_vsr_trunk_cfg* cfg, const Kind& k) {
  TrunkPlan P;
  if (!make_plan(cfg, k, &P)) return 0;
  return P.packed_bytes + sr::pack_table_bytes(P.pack_entries);
}

size_t trunk_workspace_bytes(const sr_vsr_trunk_cfg* cfg, const Kind& k, int n, int h, int w) {
  TrunkPlan P;
  if (!make_plan(cfg, k, &P) || n <= 0 || h <= 0 || w <= 0) return 0;
  return 3 * act_bytes(k, cfg->num_feat, n, h, w);
}

// make_plan or the entry point's refusal
#define TRUNK_PLAN(P, cfg, k, who) \
  SR_CHECK_ARG(make_plan(cfg, k, &P), "%s: bad config (num_feat a multiple of %d, num_block >= 0, cin_segs 1 or 2)", who, (k).lanes)

int trunk_pack(const sr_vsr_trunk_cfg* cfg, const Kind& k, const char* who, const float* const* params, void* packed_, hipStream_t stream) {
  char* const packed = (char*)packed_;
  TrunkPlan P;
  TRUNK_PLAN(P, cfg, k, who);
  SR_CHECK_ARG(params && packed, "%s: null argument", who);
  SR_CHECK_ARG(((uintptr_t)packed & 255u) == 0, "%s: packed must be 256-byte aligned", who);
  std::vector<sr::PackEntry> tab(P.convs.size());  // one launch for all images (pack_net.hip)
  for (size_t i = 0; i < P.convs.size(); ++i) {
    const TrunkConv& cp = P.convs[i];
    SR_CHECK_ARG(params[2 * i] && params[2 * i + 1], "%s: null parameter %zu", who, i);
    sr::PackEntry& e = tab[i];
    e = sr::PackEntry{};
    e.kind = 0;
    e.w[0] = params[2 * i];
    e.bias = params[2 * i + 1];
    e.out = packed + cp.w_off;
    e.bout = (float*)(packed + cp.b_off);
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
  return sr::pack_table_run(tab, packed, P.packed_bytes, k.bf16, stream);
}

// ConvResidualBlocks: `who` the entry point, `ws_query` the name of its workspace query (for the message).  The activations are
// numbered in the order they are written: 0 the first conv's output, 1 + 2 b the ReLU output of block b, 2 + 2 b its output (the
// last one is `out`).  keep = false: activation i lives in buffer i % 3 of the workspace, the rotation of sr_hip_vsr.h.  keep = true
// (include/sr_hip_vsr_bwd.h): the workspace is the caller's stack of 2 * num_block buffers and activation i stays in buffer i.
int trunk_run(const sr_vsr_trunk_cfg* cfg, const Kind& k, const char* who, const char* ws_query, const void* packed_, const void* in,
              long long in_img_stride, void* out, long long out_img_stride, int n, int h, int w, void* workspace,
              size_t workspace_bytes, hipStream_t stream, bool keep = false) {
  const char* const packed = (const char*)packed_;
  TrunkPlan P;
  TRUNK_PLAN(P, cfg, k, who);
  SR_CHECK_ARG(packed && in && out, "%s: null packed / in / out", who);
  SR_CHECK_ARG(n > 0 && h > 0 && w > 0, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
  const int nf = cfg->num_feat, mult = 16 / k.elem;
  const long long hw = (long long)h * w, feat_ns = (long long)nf * hw;
  SR_CHECK_ARG(hw * k.elem * P.cin_pad0 < (1ll << 31), "%s: image too large for 32-bit plane offsets", who);
  SR_CHECK_ARG(sr::aligned16(packed) && sr::aligned16(in) && sr::aligned16(out) && ((uintptr_t)workspace & 255u) == 0,
               "%s: packed / in / out must be 16-byte, the workspace 256-byte aligned", who);
  SR_CHECK_ARG(in_img_stride % mult == 0 && out_img_stride % mult == 0, "%s: image strides must be multiples of %d %s", who, mult, k.unit);
  SR_CHECK_ARG(n == 1 || (in_img_stride >= (long long)P.cin_pad0 * hw && out_img_stride >= feat_ns),
               "%s: an image stride is smaller than the image", who);
  const size_t one = act_bytes(k, nf, n, h, w), need = (keep ? 2 : cfg->num_block > 0 ? 3 : 0) * (keep ? cfg->num_block : 1) * one;
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    sr::set_error("%s: %s of %zu bytes, %zu needed (%s)", who, keep ? "stack" : "workspace", workspace_bytes, need, ws_query);
    return SR_ENOSPACE;
  }
  auto act = [&](int i) -> void* { return (char*)workspace + (size_t)(keep ? i : i % 3) * one; };

  const bool wino = !k.bf16 && sr::wino_f32_mode() != 0;
  size_t ci = 0;
  auto conv = [&](const void* src, long long src_ns, void* dst, long long dst_ns, float slope, const void* res1) -> int {
    const TrunkConv& cp = P.convs[ci++];
    sr_conv3x3_desc d = {};  // its pointers are float* for both element types
    d.in = (const float*)src;
    d.in_img_stride = src_ns;
    d.cin_pad = cp.cin_pad;
    d.cin_real = cp.cin;
    d.in_h = h;
    d.in_w = w;
    d.wpacked = (const float*)(packed + cp.w_off);
    d.bpacked = (const float*)(packed + cp.b_off);
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
    if (k.bf16) return sr_conv3x3_bf16(&d, stream);
    if (wino && cp.wino_off != kNoWino) {
      const int rc = sr::conv3x3_wino_f32(&d, (const float*)(packed + cp.wino_off), stream, false);
      if (rc != SR_WINO_NOT_ELIGIBLE) return rc;
    }
    return sr_conv3x3_f32(&d, stream);
  };

  const int nb = cfg->num_block;
  // main.0 + LeakyReLU(0.1)
  int rc = nb == 0 ? conv(in, in_img_stride, out, out_img_stride, 0.1f, nullptr) : conv(in, in_img_stride, act(0), feat_ns, 0.1f, nullptr);
  for (int b = 0; b < nb && rc == SR_OK; ++b) {
    void *const x = act(2 * b), *const t = act(2 * b + 1);  // the block input and relu(conv1(x))
    rc = conv(x, feat_ns, t, feat_ns, 0.f, nullptr);
    if (rc) break;
    if (b + 1 == nb)
      rc = conv(t, feat_ns, out, out_img_stride, 1.f, x);  // x + conv2(.)
    else
      rc = conv(t, feat_ns, act(2 * b + 2), feat_ns, 1.f, x);
  }
  return rc;
}

}  // namespace

// ---------------------------------------------------------------------- what vsr_bwd_ops.hip shares of the driver (vsr_trunk.h)
namespace sr {

size_t vsr_trunk_act_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w) {
  TrunkPlan P;
  if (!make_plan(cfg, kF32, &P) || n <= 0 || h <= 0 || w <= 0) return 0;
  return act_bytes(kF32, cfg->num_feat, n, h, w);
}

int vsr_trunk_keep_run(const sr_vsr_trunk_cfg* cfg, const char* who, const char* stack_query, const float* packed, const float* in,
                       long long in_img_stride, float* out, long long out_img_stride, int n, int h, int w, void* stack,
                       size_t stack_bytes, hipStream_t stream) {
  return trunk_run(cfg, kF32, who, stack_query, packed, in, in_img_stride, out, out_img_stride, n, h, w, stack, stack_bytes, stream, true);
}

}  // namespace sr

// ------------------------------------------------------------------------------------------- fp32 (include/sr_hip_vsr.h)
extern "C" int sr_vsr_prop_input_f32(const sr_vsr_prop_desc* d, void* stream) {
  return prop_input(kF32, "sr_vsr_prop_input_f32", 159, vsr_prop_input_kernel, d, (hipStream_t)stream);
}

extern "C" int sr_vsr_trunk_num_params(const sr_vsr_trunk_cfg* cfg) {
  TrunkPlan P;
  TRUNK_PLAN(P, cfg, kF32, "sr_vsr_trunk_num_params");
  return 2 * (int)P.convs.size();
}

extern "C" int sr_vsr_trunk_conv_wino(const sr_vsr_trunk_cfg* cfg, int index) {
  TrunkPlan P;
  TRUNK_PLAN(P, cfg, kF32, "sr_vsr_trunk_conv_wino");
  SR_CHECK_ARG(index >= 0 && (size_t)index < P.convs.size(), "sr_vsr_trunk_conv_wino: conv %d of %zu", index, P.convs.size());
  return P.convs[index].wino_off != kNoWino ? 1 : 0;
}

extern "C" size_t sr_vsr_trunk_packed_bytes(const sr_vsr_trunk_cfg* cfg) { return trunk_packed_bytes(cfg, kF32); }

extern "C" size_t sr_vsr_trunk_workspace_bytes(const sr_vsr_trunk_cfg* cfg, int n, int h, int w) {
  return trunk_workspace_bytes(cfg, kF32, n, h, w);
}

extern "C" int sr_vsr_trunk_pack_f32(const sr_vsr_trunk_cfg* cfg, const float* const* params, float* packed, void* stream) {
  return trunk_pack(cfg, kF32, "sr_vsr_trunk_pack_f32", params, packed, (hipStream_t)stream);
}

extern "C" int sr_vsr_trunk_f32(const sr_vsr_trunk_cfg* cfg, const float* packed, const float* in, long long in_img_stride, float* out,
                                long long out_img_stride, int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  return trunk_run(cfg, kF32, "sr_vsr_trunk_f32", "sr_vsr_trunk_workspace_bytes", packed, in, in_img_stride, out, out_img_stride, n, h, w,
                   workspace, workspace_bytes, (hipStream_t)stream);
}

// -------------------------------------------------------------------------------------- bf16 (include/sr_hip_vsr_bf16.h)
extern "C" int sr_rvsr_prop_input_bf16(const sr_rvsr_prop_desc* d, void* stream) {
  return prop_input(kBf16, "sr_rvsr_prop_input_bf16", 167, vsr_prop_input_bf16_kernel, d, (hipStream_t)stream);
}

extern "C" size_t sr_rvsr_trunk_packed_bytes_bf16(const sr_vsr_trunk_cfg* cfg) { return trunk_packed_bytes(cfg, kBf16); }

extern "C" size_t sr_rvsr_trunk_workspace_bytes_bf16(const sr_vsr_trunk_cfg* cfg, int n, int h, int w) {
  return trunk_workspace_bytes(cfg, kBf16, n, h, w);
}

extern "C" int sr_rvsr_trunk_pack_bf16(const sr_vsr_trunk_cfg* cfg, const float* const* params, void* packed, void* stream) {
  return trunk_pack(cfg, kBf16, "sr_rvsr_trunk_pack_bf16", params, packed, (hipStream_t)stream);
}

extern "C" int sr_rvsr_trunk_bf16(const sr_vsr_trunk_cfg* cfg, const void* packed, const void* in, long long in_img_stride, void* out,
                                  long long out_img_stride, int n, int h, int w, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  return trunk_run(cfg, kBf16, "sr_rvsr_trunk_bf16", "sr_rvsr_trunk_workspace_bytes_bf16", packed, in, in_img_stride, out, out_img_stride,
                   n, h, w, workspace, workspace_bytes, (hipStream_t)stream);
}
