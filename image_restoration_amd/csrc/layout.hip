// Layout conversion and weight packing kernels (HBM-bound, tiny next to the convs).
//   NCHW <-> CB8 at the module boundary (caller tensors are NCHW),
//   with the reference's pixel_unshuffle (arch_util.py:185-201) fused into the load;
//   OIHW conv weights -> MFMA A-operand image [group][cin/8][tap][group couts][8].
#include "sr_internal.h"

namespace sr {
int conv_group_couts(int cout);
}

namespace {

// One thread per destination pixel-block: 8 channels = 32 B written, 8 strided plane reads.
__global__ void nchw_to_cb8_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W, int u,
                                   int cblocks, long long dst_ns, long long total) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int HW = H * W;
  const int pix = (int)(i % HW);
  long long r = i / HW;
  const int cb = (int)(r % cblocks);
  const int n = (int)(r / cblocks);
  const int y = pix / W, x = pix - y * W;
  const int Cu = C * u * u;
  const int SH = H * u, SW = W * u;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = cb * 8 + e;
    float val = 0.f;
    if (c < Cu) {
      // pixel_unshuffle channel order: c = (c_src*u + iy)*u + ix   (arch_util.py:200-201)
      const int ix = c % u, iy = (c / u) % u, cs = c / (u * u);
      val = src[((long long)(n * C + cs) * SH + (y * u + iy)) * SW + (x * u + ix)];
    }
    v[e] = val;
  }
  float4* o = (float4*)(dst + n * dst_ns + ((long long)cb * HW + pix) * 8);
  o[0] = make_float4(v[0], v[1], v[2], v[3]);
  o[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// One thread per destination element of [N][C][H*u][W*u]; u = 1 is the plain conversion, u > 1 the
// inverse of the pixel_unshuffle channel order  c_cb8 = (c*u + iy)*u + ix.
__global__ void cb8_to_nchw_kernel(const float* __restrict__ src, long long src_ns, float* __restrict__ dst, int C, int H,
                                   int W, int u, long long total) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int SW = W * u, SH = H * u;
  const int sx = (int)(i % SW);
  long long r = i / SW;
  const int sy = (int)(r % SH);
  r /= SH;
  const int c = (int)(r % C);
  const int n = (int)(r / C);
  const int cc = (c * u + sy % u) * u + sx % u;
  const long long pix = (long long)(sy / u) * W + sx / u;
  dst[i] = src[n * src_ns + ((long long)(cc >> 3) * H * W + pix) * 8 + (cc & 7)];
}

// mode 0: thread per (co, ci, tap) of the OIHW weight, scattered into the (pre-zeroed) image
//         wp[g][cb][tap][co % gc][c8],  g = co / gc, (cb, c8) = position of ci in the CB8 source.
// mode 1: data-gradient image: "output channel" = position of ci, "input channel" = co, tap flipped.
__global__ void pack_w_kernel(const float* __restrict__ w, int cout, int cin, int first_seg, int seg, int cin_pad,
                              int mode, float* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cout * cin * 9) return;
  const int tap = i % 9;
  const int ci = (i / 9) % cin;
  const int co = i / (9 * cin);
  int pos = ci;
  if (ci >= first_seg) {
    const int r = ci - first_seg;
    pos = (first_seg + 7) / 8 * 8 + (r / seg) * ((seg + 7) / 8 * 8) + r % seg;
  }
  const float val = w[i];
  if (mode == 0) {
    const int gc = (((cout + 31) / 32 * 32) % 64 == 0) ? 64 : 32;
    const int cbs = cin_pad / 8;
    const int g = co / gc, col = co % gc;
    wp[((((long long)g * cbs + (pos >> 3)) * 9 + tap) * gc + col) * 8 + (pos & 7)] = val;
  } else {
    const int oc = cin_pad;  // output channels of the dgrad conv
    const int gc = (((oc + 31) / 32 * 32) % 64 == 0) ? 64 : 32;
    const int cbs = (cout + 7) / 8;
    const int g = pos / gc, col = pos % gc;
    wp[((((long long)g * cbs + (co >> 3)) * 9 + (8 - tap)) * gc + col) * 8 + (co & 7)] = val;
  }
}

__global__ void pack_b_kernel(const float* __restrict__ b, int cout, int cpad, float* __restrict__ bp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cpad) bp[i] = (b && i < cout) ? b[i] : 0.f;
}

}  // namespace

extern "C" int sr_nchw_to_cb8_f32(const float* src, float* dst, int N, int C, int H, int W, int unshuffle,
                                  int dst_cblocks, int64_t dst_img_stride, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(src && dst && N > 0 && C > 0 && H > 0 && W > 0, "sr_nchw_to_cb8_f32: bad argument");
  SR_CHECK_ARG(unshuffle == 1 || unshuffle == 2 || unshuffle == 4, "sr_nchw_to_cb8_f32: unshuffle must be 1, 2 or 4");
  SR_CHECK_ARG(dst_cblocks * 8 >= C * unshuffle * unshuffle, "sr_nchw_to_cb8_f32: dst_cblocks too small");
  SR_CHECK_ARG((uintptr_t)dst % 16 == 0 && dst_img_stride % 4 == 0, "sr_nchw_to_cb8_f32: dst must be 16-byte aligned");
  const long long total = (long long)N * dst_cblocks * H * W;
  hipLaunchKernelGGL(nchw_to_cb8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, dst, C, H, W,
                     unshuffle, dst_cblocks, (long long)dst_img_stride, total);
  SR_CHECK_LAUNCH("nchw_to_cb8");
  return SR_OK;
}

extern "C" int sr_cb8_to_nchw_f32(const float* src, int64_t src_img_stride, float* dst, int N, int C, int H, int W,
                                  int shuffle, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(src && dst && N > 0 && C > 0 && H > 0 && W > 0, "sr_cb8_to_nchw_f32: bad argument");
  SR_CHECK_ARG(shuffle == 1 || shuffle == 2 || shuffle == 4, "sr_cb8_to_nchw_f32: shuffle must be 1, 2 or 4");
  const long long total = (long long)N * C * H * W * shuffle * shuffle;
  hipLaunchKernelGGL(cb8_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src,
                     (long long)src_img_stride, dst, C, H, W, shuffle, total);
  SR_CHECK_LAUNCH("cb8_to_nchw");
  return SR_OK;
}

extern "C" size_t sr_conv3x3_packed_weight_floats(int cout, int cin_pad) {
  const int cp = (cout + 31) / 32 * 32;
  return (size_t)cp * (size_t)cin_pad * 9;
}

extern "C" size_t sr_conv3x3_packed_bias_floats(int cout) { return (size_t)((cout + 31) / 32 * 32); }

extern "C" int sr_conv3x3_cin_pad(int cin, int first_seg, int seg) {
  if (cin <= 0 || first_seg <= 0 || first_seg > cin) return SR_EINVAL;
  if (first_seg == cin) return (cin + 7) / 8 * 8;
  if (seg <= 0 || (cin - first_seg) % seg != 0) return SR_EINVAL;
  return (first_seg + 7) / 8 * 8 + ((cin - first_seg) / seg) * ((seg + 7) / 8 * 8);
}

extern "C" int sr_conv3x3_pack_f32(const float* weight, const float* bias, int cout, int cin, int first_seg, int seg,
                                   int mode, float* wpacked, float* bpacked, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(weight && wpacked && cout > 0 && cin > 0, "sr_conv3x3_pack_f32: bad argument");
  const int cin_pad = sr_conv3x3_cin_pad(cin, first_seg, seg);
  SR_CHECK_ARG(cin_pad > 0, "sr_conv3x3_pack_f32: cin=%d is not first_seg=%d + k*seg=%d", cin, first_seg, seg);
  SR_CHECK_ARG(mode == 0 || mode == 1, "sr_conv3x3_pack_f32: mode must be 0 or 1");
  const size_t wfloats = mode == 0 ? sr_conv3x3_packed_weight_floats(cout, cin_pad)
                                   : sr_conv3x3_packed_weight_floats(cin_pad, (cout + 7) / 8 * 8);
  if (hipMemsetAsync(wpacked, 0, wfloats * sizeof(float), stream) != hipSuccess) {
    sr::set_error("sr_conv3x3_pack_f32: memset failed");
    return SR_ELAUNCH;
  }
  const int total = cout * cin * 9;
  hipLaunchKernelGGL(pack_w_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, weight, cout, cin, first_seg,
                     seg > 0 ? seg : 1, cin_pad, mode, wpacked);
  SR_CHECK_LAUNCH("pack_w");
  if (bpacked && mode == 0) {
    const int cp = (int)sr_conv3x3_packed_bias_floats(cout);
    hipLaunchKernelGGL(pack_b_kernel, dim3((cp + 255) / 256), dim3(256), 0, stream, bias, cout, cp, bpacked);
    SR_CHECK_LAUNCH("pack_b");
  }
  return SR_OK;
}

// ---- small HBM-bound helpers of the backward pass -------------------------------------------------
namespace {

// Backward of F.interpolate(scale_factor=2, mode='nearest') (rrdbnet_arch.py:116-117): every source pixel
// fed a 2x2 block, so its gradient is the 2x2 sum; optionally followed by the LeakyReLU backward of the
// activation that produced the source (mask tensor has the destination's shape).
// One thread per destination float4 (half a pixel-block).
__global__ void up2x_bwd_kernel(const float* __restrict__ g, long long g_ns, float* __restrict__ dst, long long dst_ns,
                                const float* __restrict__ mask, long long mask_ns, float slope, int cblocks, int h, int w,
                                long long total) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int half = (int)(i & 1);
  long long r = i >> 1;
  const int x = (int)(r % w);
  r /= w;
  const int y = (int)(r % h);
  r /= h;
  const int cb = (int)(r % cblocks);
  const int n = (int)(r / cblocks);
  const int W2 = 2 * w;
  const float* s = g + n * g_ns + (((long long)cb * 2 * h + 2 * y) * W2 + 2 * x) * 8 + half * 4;
  const float4 a = *(const float4*)s, b = *(const float4*)(s + 8), c = *(const float4*)(s + (long long)W2 * 8),
               d = *(const float4*)(s + (long long)W2 * 8 + 8);
  float4 v = make_float4(a.x + b.x + c.x + d.x, a.y + b.y + c.y + d.y, a.z + b.z + c.z + d.z, a.w + b.w + c.w + d.w);
  const long long off = (((long long)cb * h + y) * w + x) * 8 + half * 4;
  if (mask) {
    const float4 m = *(const float4*)(mask + n * mask_ns + off);
    v.x = m.x > 0.f ? v.x : v.x * slope;
    v.y = m.y > 0.f ? v.y : v.y * slope;
    v.z = m.z > 0.f ? v.z : v.z * slope;
    v.w = m.w > 0.f ? v.w : v.w * slope;
  }
  *(float4*)(dst + n * dst_ns + off) = v;
}

// dst = a*dst + b*src on CB8 windows (float4 granularity).
__global__ void cb8_axpby_kernel(float* __restrict__ dst, long long dst_ns, const float* __restrict__ src,
                                 long long src_ns, float a, float b, long long per_img4, long long total) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long n = i / per_img4, o = (i % per_img4) * 4;
  float4* d = (float4*)(dst + n * dst_ns + o);
  const float4 s = *(const float4*)(src + n * src_ns + o);
  float4 v = *d;
  v.x = a * v.x + b * s.x;
  v.y = a * v.y + b * s.y;
  v.z = a * v.z + b * s.z;
  v.w = a * v.w + b * s.w;
  *d = v;
}

}  // namespace

extern "C" int sr_upsample2x_bwd_f32(const float* g, int64_t g_img_stride, float* dst, int64_t dst_img_stride,
                                     const float* mask, int64_t mask_img_stride, float mask_slope, int n, int cblocks,
                                     int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(g && dst && n > 0 && cblocks > 0 && h > 0 && w > 0, "sr_upsample2x_bwd_f32: bad argument");
  SR_CHECK_ARG((uintptr_t)g % 16 == 0 && (uintptr_t)dst % 16 == 0 && (uintptr_t)mask % 16 == 0 && g_img_stride % 4 == 0 &&
                   dst_img_stride % 4 == 0 && (!mask || mask_img_stride % 4 == 0),
               "sr_upsample2x_bwd_f32: g, dst and mask must be 16-byte aligned");
  const long long total = (long long)n * cblocks * h * w * 2;
  hipLaunchKernelGGL(up2x_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, g,
                     (long long)g_img_stride, dst, (long long)dst_img_stride, mask, (long long)mask_img_stride,
                     mask_slope, cblocks, h, w, total);
  SR_CHECK_LAUNCH("up2x_bwd");
  return SR_OK;
}

extern "C" int sr_cb8_axpby_f32(float* dst, int64_t dst_img_stride, const float* src, int64_t src_img_stride, float a,
                                float b, int n, int cblocks, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(dst && src && n > 0 && cblocks > 0 && h > 0 && w > 0, "sr_cb8_axpby_f32: bad argument");
  SR_CHECK_ARG((uintptr_t)dst % 16 == 0 && (uintptr_t)src % 16 == 0 && dst_img_stride % 4 == 0 && src_img_stride % 4 == 0,
               "sr_cb8_axpby_f32: dst and src must be 16-byte aligned");
  const long long per_img4 = (long long)cblocks * h * w * 2;
  const long long total = per_img4 * n;
  hipLaunchKernelGGL(cb8_axpby_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, dst,
                     (long long)dst_img_stride, src, (long long)src_img_stride, a, b, per_img4, total);
  SR_CHECK_LAUNCH("cb8_axpby");
  return SR_OK;
}

// ---- 4x4 / stride-2 conv weights: four parity-pass images of a 2x2 tap grid -------------------------
namespace {
// thread per (co, ci, dy, dx) of the OIHW [cout][cin][4][4] weight.
//   mode 0 (forward):  pass = (ry, rx) with ry = 1 - (dy & 1), tap ty = dy >> 1          (see sr_conv4x4s2_f32)
//   mode 1 (dgrad):    pass = (py, px) with py = 1 - (dy & 1), tap ty = (3 - dy) >> 1, channel roles swapped
__global__ void pack_w4_kernel(const float* __restrict__ w, int cout, int cin, int cin_pad, int mode,
                               float* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cout * cin * 16) return;
  const int dx = i & 3, dy = (i >> 2) & 3;
  const int ci = (i >> 4) % cin, co = i / (16 * cin);
  const float val = w[i];
  const int pass = (1 - (dy & 1)) * 2 + (1 - (dx & 1));
  if (mode == 0) {
    const int tap = (dy >> 1) * 2 + (dx >> 1);
    const int gc = (((cout + 31) / 32 * 32) % 64 == 0) ? 64 : 32;
    const int G = ((cout + 31) / 32 * 32) / gc, cbs = cin_pad / 8;
    const int g = co / gc, col = co % gc;
    wp[(((((long long)pass * G + g) * cbs + (ci >> 3)) * 4 + tap) * gc + col) * 8 + (ci & 7)] = val;
  } else {
    const int tap = ((3 - dy) >> 1) * 2 + ((3 - dx) >> 1);
    const int oc = cin_pad;
    const int gc = (((oc + 31) / 32 * 32) % 64 == 0) ? 64 : 32;
    const int G = ((oc + 31) / 32 * 32) / gc, cbs = (cout + 7) / 8;
    const int g = ci / gc, col = ci % gc;
    wp[(((((long long)pass * G + g) * cbs + (co >> 3)) * 4 + tap) * gc + col) * 8 + (co & 7)] = val;
  }
}
}  // namespace

extern "C" size_t sr_conv4x4s2_packed_weight_floats(int cout, int cin, int mode) {
  const int cin_pad = (cin + 7) / 8 * 8;
  if (mode == 0) return (size_t)((cout + 31) / 32 * 32) * cin_pad * 16;
  return (size_t)((cin_pad + 31) / 32 * 32) * ((cout + 7) / 8 * 8) * 16;
}

extern "C" int sr_conv4x4s2_pack_f32(const float* weight, const float* bias, int cout, int cin, int mode, float* wpacked,
                                     float* bpacked, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(weight && wpacked && cout > 0 && cin > 0 && (mode == 0 || mode == 1), "sr_conv4x4s2_pack_f32: bad argument");
  const size_t wfloats = sr_conv4x4s2_packed_weight_floats(cout, cin, mode);
  if (hipMemsetAsync(wpacked, 0, wfloats * sizeof(float), stream) != hipSuccess) {
    sr::set_error("sr_conv4x4s2_pack_f32: memset failed");
    return SR_ELAUNCH;
  }
  const int total = cout * cin * 16;
  hipLaunchKernelGGL(pack_w4_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, weight, cout, cin,
                     (cin + 7) / 8 * 8, mode, wpacked);
  SR_CHECK_LAUNCH("pack_w4");
  if (bpacked && mode == 0) {
    const int cp = (int)sr_conv3x3_packed_bias_floats(cout);
    hipLaunchKernelGGL(pack_b_kernel, dim3((cp + 255) / 256), dim3(256), 0, stream, bias, cout, cp, bpacked);
    SR_CHECK_LAUNCH("pack_b");
  }
  return SR_OK;
}


// ---- data-gradient weights of a residual dense block as a TRANSPOSED dense block ---------------------------
// Backward of ResidualDenseBlock.forward (rrdbnet_arch.py:32-39) is itself a dense block over the gradient concat
// [dY5 | dY4 | dY3 | dY2 | dY1]:  the gradient of slice s (s = 4..1: x4..x1, s = 0: x) is ONE 3x3 conv whose input
// is every dY_k with k > s and whose weights are W_k[:, slice s]^T with flipped taps (W5's part carries the 0.2 /
// 0.04 residual scale).  Same shapes as the forward convs (64->32, 96->32, 128->32, 160->32, 192->64), every
// output written once: no read-modify-write accumulation, no K = 288 launches.
namespace {
struct DensePackParams {
  const float* w[5];  // conv1..conv5 OIHW
  float* out;
  int nf, gc, nfp, gcp, s;
  float scale5;
};
// thread per (k, co, ci_local, tap) with k = s+1..5; element counts are prefix-summed on the fly
__global__ void pack_dense_dgrad_kernel(const DensePackParams p) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int slice = p.s == 0 ? p.nf : p.gc;
  const int slice0 = p.s == 0 ? 0 : p.nf + (p.s - 1) * p.gc;
  const int cin_pad = p.nfp + (4 - p.s) * p.gcp;  // D-order input channels of this step (s >= 1: dY5..dY_{s+1}); s = 0: all
  const int cinp = p.s == 0 ? p.nfp + 4 * p.gcp : cin_pad;
  for (int k = 5; k > p.s; --k) {
    const int cout_k = k == 5 ? p.nf : p.gc, cin_k = p.nf + (k - 1) * p.gc;
    const long long cnt = (long long)cout_k * slice * 9;
    if (i < cnt) {
      const int tap = (int)(i % 9);
      const int cil = (int)((i / 9) % slice);
      const int co = (int)(i / (9LL * slice));
      float v = p.w[k - 1][((long long)co * cin_k + slice0 + cil) * 9 + tap];
      if (k == 5) v *= p.scale5;
      const int pos = k == 5 ? co : p.nfp + (4 - k) * p.gcp + co;
      const int gcw = (((slice + 31) / 32 * 32) % 64 == 0) ? 64 : 32;
      const int cbs = cinp / 8;
      const int g = cil / gcw, col = cil % gcw;
      p.out[((((long long)g * cbs + (pos >> 3)) * 9 + (8 - tap)) * gcw + col) * 8 + (pos & 7)] = v;
      return;
    }
    i -= cnt;
  }
}
}  // namespace

namespace sr {
size_t rdb_dgrad_step_floats(int nf, int gc, int s) {
  const int nfp = (nf + 7) / 8 * 8, gcp = (gc + 7) / 8 * 8;
  const int slice = s == 0 ? nf : gc;
  const int cinp = nfp + (4 - s) * gcp;
  return sr_conv3x3_packed_weight_floats(slice, cinp);
}
int rdb_pack_dgrad_step(const float* const w[5], int nf, int gc, int s, float scale5, float* out, hipStream_t stream) {
  const size_t floats = rdb_dgrad_step_floats(nf, gc, s);
  if (hipMemsetAsync(out, 0, floats * sizeof(float), stream) != hipSuccess) {
    set_error("rdb_pack_dgrad_step: memset failed");
    return SR_ELAUNCH;
  }
  DensePackParams p;
  for (int i = 0; i < 5; ++i) p.w[i] = w[i];
  p.out = out;
  p.nf = nf;
  p.gc = gc;
  p.nfp = (nf + 7) / 8 * 8;
  p.gcp = (gc + 7) / 8 * 8;
  p.s = s;
  p.scale5 = scale5;
  const int slice = s == 0 ? nf : gc;
  long long total = 0;
  for (int k = 5; k > s; --k) total += (long long)(k == 5 ? nf : gc) * slice * 9;
  hipLaunchKernelGGL(pack_dense_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p);
  SR_CHECK_LAUNCH("pack_dense_dgrad");
  return SR_OK;
}
}  // namespace sr
