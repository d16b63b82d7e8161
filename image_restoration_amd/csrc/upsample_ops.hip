// The two operations MSRResNet (basicsr/archs/srresnet_arch.py:9-68) needs beyond the 3x3 convs:
//  - nn.PixelShuffle(r) / its inverse, r in {2, 3}, CB8 -> CB8.  LeakyReLU commutes with the permutation, so the upconv's
//    epilogue applies it and the consuming conv's data-gradient epilogue applies its mask: both kernels are pure moves.
//  - F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False), s in {2, 3, 4}, NCHW fp32 (the `base` term),
//    and its adjoint in gather form: every dx element sums its own output window in a fixed order, no atomics, so the
//    backward is bit-reproducible.
// All four are HBM-bound: one thread per destination pixel, whole 32-byte CB8 pixels stored (two 16-byte stores).
#include "sr_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// dst[n][c][r*h + i][r*w + j] = src[n][c*r*r + i*r + j][h][w]   (torch.nn.PixelShuffle channel order)
// src: ceil(r*r*C/8) CB8 blocks at H x W; dst: ceil(C/8) blocks at rH x rW; pad channels of dst are written 0.
template <int R>
__global__ __launch_bounds__(256) void cb8_pixel_shuffle_kernel(const float* __restrict__ src, long long src_ns,
                                                                float* __restrict__ dst, long long dst_ns, int C, int dblocks,
                                                                int H, int W) {
  const int OW = W * R;
  const long long OHW = (long long)H * R * OW;
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= OHW) return;
  const int n = blockIdx.y / dblocks, db = blockIdx.y - n * dblocks;
  const int oy = (int)(pix / OW), ox = (int)(pix - (long long)oy * OW);
  const int h = oy / R, i = oy - h * R, w = ox / R, j = ox - w * R;
  const long long HW = (long long)H * W;
  const float* s = src + n * src_ns + ((long long)h * W + w) * 8;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = db * 8 + k;
    const int sc = c * R * R + i * R + j;
    v[k] = c < C ? s[(sc >> 3) * HW * 8 + (sc & 7)] : 0.f;
  }
  f32x4* d = (f32x4*)(dst + n * dst_ns + ((long long)db * OHW + pix) * 8);
  d[0] = f32x4{v[0], v[1], v[2], v[3]};
  d[1] = f32x4{v[4], v[5], v[6], v[7]};
}

// The inverse (torch.nn.PixelUnshuffle(r)): dst[n][c*r*r + i*r + j][h][w] = src[n][c][r*h + i][r*w + j]
// src: ceil(C/8) blocks at rH x rW; dst: ceil(r*r*C/8) blocks at H x W; pad channels of dst are written 0.
template <int R>
__global__ __launch_bounds__(256) void cb8_pixel_unshuffle_kernel(const float* __restrict__ src, long long src_ns,
                                                                  float* __restrict__ dst, long long dst_ns, int C, int dblocks,
                                                                  int H, int W) {
  const long long HW = (long long)H * W;
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int n = blockIdx.y / dblocks, db = blockIdx.y - n * dblocks;
  const int h = (int)(pix / W), w = (int)(pix - (long long)h * W);
  const int OW = W * R;
  const long long OHW = HW * R * R;
  const float* s = src + n * src_ns;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int sc = db * 8 + k;
    const int c = sc / (R * R), rem = sc - c * R * R;
    const int i = rem / R, j = rem - i * R;
    v[k] = sc < C * R * R ? s[((c >> 3) * OHW + (long long)(h * R + i) * OW + (w * R + j)) * 8 + (c & 7)] : 0.f;
  }
  f32x4* d = (f32x4*)(dst + n * dst_ns + ((long long)db * HW + pix) * 8);
  d[0] = f32x4{v[0], v[1], v[2], v[3]};
  d[1] = f32x4{v[4], v[5], v[6], v[7]};
}

// torch's source index for an integer scale_factor, align_corners=False (area_pixel_compute_source_index with
// scale = 1/s in fp32): src = max((dst + 0.5) / s - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, size - 1), lambda = src - i0.
struct Tap {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Tap src_tap(int o, float inv_s, int size) {
  float f = inv_s * ((float)o + 0.5f) - 0.5f;
  f = f < 0.f ? 0.f : f;
  Tap t;
  t.i0 = (int)f;
  t.i1 = t.i0 < size - 1 ? t.i0 + 1 : t.i0;
  t.l1 = f - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// y[n][c][oy][ox] (+)= l0y*(l0x*x[y0][x0] + l1x*x[y0][x1]) + l1y*(l0x*x[y1][x0] + l1x*x[y1][x1])
__global__ __launch_bounds__(256) void bilinear_up_nchw_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                               int S, float inv_s, int accumulate) {
  const int OW = W * S;
  const long long OHW = (long long)H * S * OW;
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= OHW) return;
  const long long plane = blockIdx.y;
  const int oy = (int)(pix / OW), ox = (int)(pix - (long long)oy * OW);
  const Tap ty = src_tap(oy, inv_s, H), tx = src_tap(ox, inv_s, W);
  const float* p = x + plane * H * W;
  const float* r0 = p + (long long)ty.i0 * W;
  const float* r1 = p + (long long)ty.i1 * W;
  const float top = tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1];
  const float bot = tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1];
  float v = ty.l0 * top + ty.l1 * bot;
  float* o = y + plane * OHW + pix;
  if (accumulate) v = *o + v;
  *o = v;
}

// Weight of input index `i` in output index `o`'s interpolation (both taps may land on `i` at the last row / column).
__device__ __forceinline__ float tap_weight(int o, int i, float inv_s, int size) {
  const Tap t = src_tap(o, inv_s, size);
  return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

// Adjoint, gather form: dx[n][c][iy][ix] (+)= sum_oy wy(oy) * (sum_ox wx(ox) * g[oy][ox]) over the only output rows / columns
// whose taps can reach iy / ix: [s*iy - s, s*iy + 2s) (their source index lies in [iy - 1, iy + 1)).  Fixed order, no atomics.
__global__ __launch_bounds__(256) void bilinear_up_nchw_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, int H, int W,
                                                                   int S, float inv_s, int accumulate) {
  const long long HW = (long long)H * W;
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const long long plane = blockIdx.y;
  const int iy = (int)(pix / W), ix = (int)(pix - (long long)iy * W);
  const int OH = H * S, OW = W * S;
  const int y_lo = max(0, S * iy - S), y_hi = min(OH, S * iy + 2 * S);
  const int x_lo = max(0, S * ix - S), x_hi = min(OW, S * ix + 2 * S);
  const float* gp = g + plane * OH * OW;
  float acc = 0.f;
  for (int oy = y_lo; oy < y_hi; ++oy) {
    const float wy = tap_weight(oy, iy, inv_s, H);
    if (wy == 0.f) continue;
    const float* row = gp + (long long)oy * OW;
    float racc = 0.f;
    for (int ox = x_lo; ox < x_hi; ++ox) {
      const float wx = tap_weight(ox, ix, inv_s, W);
      if (wx != 0.f) racc += wx * row[ox];
    }
    acc += wy * racc;
  }
  float* o = dx + plane * HW + pix;
  if (accumulate) acc = *o + acc;
  *o = acc;
}

void record(hipStream_t stream, int id, int cin, int cout, int n, int h, int w, double bytes) {
  sr_launch_record r = {};
  r.kernel_id = id;
  r.cin = cin;
  r.cout = cout;
  r.n = n;
  r.h = h;
  r.w = w;
  r.bytes = bytes;
  sr::prof_begin(stream, r);
}

int shuffle_common(const float* src, int64_t src_ns, float* dst, int64_t dst_ns, int n, int C, int H, int W, int r, int inverse,
                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = inverse ? "sr_cb8_pixel_unshuffle_f32" : "sr_cb8_pixel_shuffle_f32";
  SR_CHECK_ARG(src && dst, "%s: null pointer", who);
  SR_CHECK_ARG(r == 2 || r == 3, "%s: r=%d must be 2 or 3", who, r);
  SR_CHECK_ARG(n > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape n=%d C=%d %dx%d", who, n, C, H, W);
  const int small_blocks = (C + 7) / 8, big_blocks = (C * r * r + 7) / 8;
  const int sblocks = inverse ? small_blocks : big_blocks, dblocks = inverse ? big_blocks : small_blocks;
  const long long HW = (long long)H * W, OHW = HW * r * r;
  const long long src_min = (long long)sblocks * (inverse ? OHW : HW) * 8, dst_min = (long long)dblocks * (inverse ? HW : OHW) * 8;
  SR_CHECK_ARG(src_ns >= src_min && dst_ns >= dst_min, "%s: image strides %lld / %lld below %lld / %lld", who, (long long)src_ns,
               (long long)dst_ns, src_min, dst_min);
  SR_CHECK_ARG((long long)n * dblocks <= 65535, "%s: n * destination blocks = %lld exceeds one launch", who, (long long)n * dblocks);
  SR_CHECK_ARG(((uintptr_t)dst % 16) == 0, "%s: dst must be 16-byte aligned", who);
  const long long pixels = inverse ? HW : OHW;
  SR_CHECK_ARG(pixels / 256 < (1LL << 31) - 1, "%s: image too large", who);
  const bool prof = sr::prof_on();
  if (prof)
    record(stream, inverse ? 71 : 70, inverse ? C : C * r * r, inverse ? C * r * r : C, n, inverse ? H : H * r, inverse ? W : W * r,
           4.0 * n * ((double)C * OHW + (double)dblocks * 8 * (inverse ? HW : OHW)));
  const dim3 grid((unsigned)((pixels + 255) / 256), (unsigned)(n * dblocks));
  if (inverse) {
    if (r == 2)
      hipLaunchKernelGGL(cb8_pixel_unshuffle_kernel<2>, grid, dim3(256), 0, stream, src, src_ns, dst, dst_ns, C, dblocks, H, W);
    else
      hipLaunchKernelGGL(cb8_pixel_unshuffle_kernel<3>, grid, dim3(256), 0, stream, src, src_ns, dst, dst_ns, C, dblocks, H, W);
  } else {
    if (r == 2)
      hipLaunchKernelGGL(cb8_pixel_shuffle_kernel<2>, grid, dim3(256), 0, stream, src, src_ns, dst, dst_ns, C, dblocks, H, W);
    else
      hipLaunchKernelGGL(cb8_pixel_shuffle_kernel<3>, grid, dim3(256), 0, stream, src, src_ns, dst, dst_ns, C, dblocks, H, W);
  }
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}

int bilinear_common(const float* src, float* dst, int n, int C, int H, int W, int s, int accumulate, int backward, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = backward ? "sr_bilinear_up_bwd_f32" : "sr_bilinear_up_f32";
  SR_CHECK_ARG(src && dst, "%s: null pointer", who);
  SR_CHECK_ARG(s >= 2 && s <= 4, "%s: scale %d must be 2, 3 or 4", who, s);
  SR_CHECK_ARG(n > 0 && C > 0 && H > 0 && W > 0 && (long long)n * C <= 65535, "%s: bad shape n=%d C=%d %dx%d", who, n, C, H, W);
  const long long HW = (long long)H * W, OHW = HW * s * s;
  SR_CHECK_ARG((long long)H * s < (1LL << 30) && (long long)W * s < (1LL << 30) && OHW / 256 < (1LL << 31) - 1, "%s: image too large",
               who);
  const long long pixels = backward ? HW : OHW;
  const bool prof = sr::prof_on();
  if (prof)
    record(stream, backward ? 73 : 72, C, C, n, backward ? H : H * s, backward ? W : W * s,
           4.0 * n * C * ((double)HW + (double)OHW + (accumulate ? (double)pixels : 0.0)));
  const dim3 grid((unsigned)((pixels + 255) / 256), (unsigned)(n * C));
  const float inv_s = (float)(1.0 / s);
  if (backward)
    hipLaunchKernelGGL(bilinear_up_nchw_bwd_kernel, grid, dim3(256), 0, stream, src, dst, H, W, s, inv_s, accumulate);
  else
    hipLaunchKernelGGL(bilinear_up_nchw_kernel, grid, dim3(256), 0, stream, src, dst, H, W, s, inv_s, accumulate);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}

}  // namespace

extern "C" int sr_cb8_pixel_shuffle_f32(const float* src, int64_t src_img_stride, float* dst, int64_t dst_img_stride, int n, int c,
                                        int h, int w, int r, void* stream) {
  return shuffle_common(src, src_img_stride, dst, dst_img_stride, n, c, h, w, r, 0, stream);
}

extern "C" int sr_cb8_pixel_unshuffle_f32(const float* src, int64_t src_img_stride, float* dst, int64_t dst_img_stride, int n, int c,
                                          int h, int w, int r, void* stream) {
  return shuffle_common(src, src_img_stride, dst, dst_img_stride, n, c, h, w, r, 1, stream);
}

extern "C" int sr_bilinear_up_f32(const float* x, float* y, int n, int c, int h, int w, int s, int accumulate, void* stream) {
  return bilinear_common(x, y, n, c, h, w, s, accumulate, 0, stream);
}

extern "C" int sr_bilinear_up_bwd_f32(const float* g, float* dx, int n, int c, int h, int w, int s, int accumulate, void* stream) {
  return bilinear_common(g, dx, n, c, h, w, s, accumulate, 1, stream);
}
