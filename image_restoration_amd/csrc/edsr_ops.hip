// EDSR (include/sr_hip_edsr.h): nn.PixelShuffle on CB16 bf16 activations and the two image shifts at the network's ends.
//
// The convolutions of EDSR are the existing sr_conv3x3_f32 / sr_conv3x3_bf16; what the bf16 forward lacked is the shuffle
// between the upsampling convs (the fp32 path has sr_cb8_pixel_shuffle_f32) and the (x - mean) * img_range input shift in one
// pass with the layout conversion.
#include "sr_internal.h"
#include "../../include/sr_hip_edsr.h"

namespace {
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float float4_t __attribute__((ext_vector_type(4)));

void prof_rec(hipStream_t stream, int id, int cin, int cout, int n, int h, int w, double bytes) {
  sr_launch_record r = {};
  r.kernel_id = id;
  r.cin = cin;
  r.cout = cout;
  r.n = n;
  r.h = h;
  r.w = w;
  r.flops = 0.0;
  r.bytes = bytes;
  sr::prof_begin(stream, r);
}

// One workgroup moves the R*R source channel blocks that make up ONE destination channel block, for kShufTile pixels of one
// source row.  The 16 channels of a destination pixel lie R*R apart in the source, so either the loads or the stores would be
// 2-byte accesses if a thread went straight from global to global.  Here both sides are 16-byte accesses in runs of whole rows
// (source: kShufTile * 32 bytes per channel block; destination: R * kShufTile * 32 bytes per output row) and the permutation
// itself happens in the LDS: 16-byte writes in source order, 2-byte gathers in destination order.
constexpr int kShufTile = 64;

struct ShufParams {
  const __bf16* src;
  __bf16* dst;
  long long src_ns, dst_ns;
  int c, h, w, src_cb, dst_cb;
};

template <int R>
__global__ __launch_bounds__(256) void cb16_pixel_shuffle_kernel(const ShufParams p) {
  constexpr int RR = R * R;
  __shared__ __attribute__((aligned(16))) __bf16 tile[RR * kShufTile * 16];
  const int x0 = blockIdx.x * kShufTile, y = blockIdx.y;
  const int n = blockIdx.z / p.dst_cb, cbd = blockIdx.z - n * p.dst_cb;
  const int tw = min(kShufTile, p.w - x0);
  const __bf16* src = p.src + n * p.src_ns;
  // source -> LDS: item = (k, x, half), x fastest within a channel block
  for (int it = threadIdx.x; it < RR * kShufTile * 2; it += 256) {
    const int half = it & 1, x = (it >> 1) % kShufTile, k = it / (2 * kShufTile);
    const int sb = cbd * RR + k;
    if (x < tw && sb < p.src_cb) {
      const bf16x8_t v = *(const bf16x8_t*)(src + (((long long)sb * p.h + y) * p.w + x0 + x) * 16 + half * 8);
      *(bf16x8_t*)(tile + (k * kShufTile + x) * 16 + half * 8) = v;
    }
  }
  __syncthreads();
  // LDS -> destination: item = (i, X, half), X = R * x + j the column within the tile's output rows
  __bf16* dst = p.dst + n * p.dst_ns;
  const int H2 = p.h * R, W2 = p.w * R;
  for (int it = threadIdx.x; it < R * R * kShufTile * 2; it += 256) {
    const int half = it & 1, X = (it >> 1) % (R * kShufTile), i = it / (2 * R * kShufTile);
    const int x = X / R, j = X - x * R;
    if (x >= tw) continue;
    bf16x8_t v;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int cl = half * 8 + q;                 // channel within the destination block
      const int ch = cl * RR + i * R + j;          // channel within the RR source blocks
      const __bf16 e = tile[((ch >> 4) * kShufTile + x) * 16 + (ch & 15)];
      v[q] = (cbd * 16 + cl < p.c) ? e : (__bf16)0.f;
    }
    *(bf16x8_t*)(dst + (((long long)cbd * H2 + y * R + i) * W2 + (long long)x0 * R + X) * 16 + half * 8) = v;
  }
}

// (x - mean[c]) * range of a 3-channel NCHW fp32 image into one channel block (CB8 fp32 or CB16 bf16, both 32-byte pixels);
// the pad channels are written as zero.  One thread per pixel: three coalesced 4-byte loads, two 16-byte stores.
template <bool BF16>
__global__ void edsr_shift_in_kernel(const float* __restrict__ x, void* __restrict__ dst_, long long dst_ns, float m0, float m1,
                                     float m2, float range, long long hw, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long n = i / hw, pix = i - n * hw;
  const float* s = x + n * 3 * hw + pix;
  const float a = (s[0] - m0) * range, b = (s[hw] - m1) * range, c = (s[2 * hw] - m2) * range;
  if (BF16) {
    __bf16* d = (__bf16*)dst_ + n * dst_ns + pix * 16;
    bf16x8_t lo = {}, hi = {};
    lo[0] = (__bf16)a;
    lo[1] = (__bf16)b;
    lo[2] = (__bf16)c;
    *(bf16x8_t*)d = lo;
    *(bf16x8_t*)(d + 8) = hi;
  } else {
    float* d = (float*)dst_ + n * dst_ns + pix * 8;
    const float4_t lo = {a, b, c, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    *(float4_t*)d = lo;
    *(float4_t*)(d + 4) = hi;
  }
}

// y = y / range + mean[c] in place on a 3-channel NCHW fp32 image
__global__ void edsr_shift_out_kernel(float* __restrict__ y, float m0, float m1, float m2, float range, long long hw,
                                      long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)((i / hw) % 3);
  const float m = c == 0 ? m0 : (c == 1 ? m1 : m2);
  y[i] = y[i] / range + m;
}

int shift_in(const float* x, void* dst, int64_t dst_img_stride, const float* mean, float range, int n, int h, int w, bool bf16,
             hipStream_t stream, const char* who) {
  SR_CHECK_ARG(x && dst && mean && n > 0 && h > 0 && w > 0, "%s: bad argument", who);
  SR_CHECK_ARG((uintptr_t)dst % 16 == 0 && dst_img_stride % 8 == 0, "%s: dst must be 16-byte aligned", who);
  const long long hw = (long long)h * w, total = hw * n;
  SR_CHECK_ARG(dst_img_stride >= hw * (bf16 ? 16 : 8), "%s: dst_img_stride %lld is smaller than one channel block", who,
               (long long)dst_img_stride);
  SR_CHECK_ARG((total + 255) / 256 < (1LL << 31), "%s: too many pixels", who);
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 99, 3, 3, n, h, w, total * (12.0 + 32.0));
  if (bf16)
    hipLaunchKernelGGL(edsr_shift_in_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, dst,
                       (long long)dst_img_stride, mean[0], mean[1], mean[2], range, hw, total);
  else
    hipLaunchKernelGGL(edsr_shift_in_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, dst,
                       (long long)dst_img_stride, mean[0], mean[1], mean[2], range, hw, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}
}  // namespace

extern "C" int sr_cb16_pixel_shuffle_bf16(const void* src, int64_t src_img_stride, void* dst, int64_t dst_img_stride, int n, int c,
                                          int h, int w, int r, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(src && dst && n > 0 && c > 0 && h > 0 && w > 0, "sr_cb16_pixel_shuffle_bf16: bad argument");
  SR_CHECK_ARG(r == 2 || r == 3, "sr_cb16_pixel_shuffle_bf16: r must be 2 or 3, got %d", r);
  SR_CHECK_ARG((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0 && src_img_stride % 8 == 0 && dst_img_stride % 8 == 0,
               "sr_cb16_pixel_shuffle_bf16: src and dst must be 16-byte aligned");
  ShufParams p;
  p.src = (const __bf16*)src;
  p.dst = (__bf16*)dst;
  p.src_ns = src_img_stride;
  p.dst_ns = dst_img_stride;
  p.c = c;
  p.h = h;
  p.w = w;
  p.src_cb = (int)(((long long)c * r * r + 15) / 16);
  p.dst_cb = (c + 15) / 16;
  const long long hw = (long long)h * w;
  SR_CHECK_ARG(src_img_stride >= hw * 16 * p.src_cb && dst_img_stride >= hw * r * r * 16 * p.dst_cb,
               "sr_cb16_pixel_shuffle_bf16: an image stride is smaller than the image");
  const long long gz = (long long)n * p.dst_cb;
  SR_CHECK_ARG(h <= 65535 && gz <= 65535, "sr_cb16_pixel_shuffle_bf16: h and n * ceil(c / 16) must not exceed 65535");
  const dim3 grid((unsigned)((w + kShufTile - 1) / kShufTile), (unsigned)h, (unsigned)gz);
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 98, c * r * r, c, n, h * r, w * r, 32.0 * n * hw * (p.src_cb + (double)r * r * p.dst_cb));
  if (r == 2)
    hipLaunchKernelGGL(cb16_pixel_shuffle_kernel<2>, grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(cb16_pixel_shuffle_kernel<3>, grid, dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_cb16_pixel_shuffle_bf16");
  return SR_OK;
}

extern "C" int sr_edsr_shift_in_f32(const float* x, float* dst, int64_t dst_img_stride, const float* mean, float range, int n, int h,
                                    int w, void* stream) {
  return shift_in(x, dst, dst_img_stride, mean, range, n, h, w, false, (hipStream_t)stream, "sr_edsr_shift_in_f32");
}

extern "C" int sr_edsr_shift_in_bf16(const float* x, void* dst, int64_t dst_img_stride, const float* mean, float range, int n, int h,
                                     int w, void* stream) {
  return shift_in(x, dst, dst_img_stride, mean, range, n, h, w, true, (hipStream_t)stream, "sr_edsr_shift_in_bf16");
}

extern "C" int sr_edsr_shift_out_f32(float* y, const float* mean, float range, int n, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(y && mean && n > 0 && h > 0 && w > 0, "sr_edsr_shift_out_f32: bad argument");
  SR_CHECK_ARG(range != 0.f, "sr_edsr_shift_out_f32: range must not be 0");
  const long long hw = (long long)h * w, total = hw * 3 * n;
  SR_CHECK_ARG((total + 255) / 256 < (1LL << 31), "sr_edsr_shift_out_f32: too many pixels");
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 100, 3, 3, n, h, w, total * 8.0);
  hipLaunchKernelGGL(edsr_shift_out_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, y, mean[0], mean[1],
                     mean[2], range, hw, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_edsr_shift_out_f32");
  return SR_OK;
}
