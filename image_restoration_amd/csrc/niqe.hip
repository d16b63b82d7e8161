// NIQE (basicsr/metrics/niqe.py:65-189) on the device: the Y image of an NCHW network output, and per block the five
// moments of the AGGD fits; the host (metrics/niqe.py) turns moments into features and the score.
//
// Float32-emulation contract: the Y and MSCN values are the reference's float32 values bit for bit.  Every float32
// operation below is the one numpy performs (IEEE division: __fdiv_rn; square root: the fp64 root rounded; -ffp-contract=off
// keeps products and sums apart), the 49-tap convolutions sum in float64 like scipy.ndimage.convolve and are rounded to
// float32 once.  The host restatement sums the taps in the same order, so host and device MSCN agree bit for bit too.
#include "sr_internal.h"

namespace {
constexpr int kBlock = 96;  // scale-1 block side; scale 2 uses kBlock / 2 on the half-size image

struct NiqeWin {
  double w[49];  // the 7x7 window, flipped (w[a*7+b] = window[6-a][6-b]): convolution as a correlation over the tile
};

__device__ __forceinline__ float quant_u8(float v) { return rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }  // tensor2img

// Y of the quantised image (metric_util.to_y_channel -> bgr2ycbcr(y_only=True)): f32(u) / 255 in f32, the dot product
// with (24.966, 128.553, 65.481) over (B, G, R) plus 16 in float64 in numpy's order, / 255, rounded to f32, * 255 in f32.
// Grey (c == 1): to_y_channel's f32(u) / 255 * 255.  Cropped to yh x yw at (crop, crop).
__global__ __launch_bounds__(256) void niqe_luma_kernel(const float* __restrict__ img, int c, int h, int w, int crop,
                                                        float* __restrict__ y, int yh, int yw, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int col = (int)(i % yw), row = (int)((i / yw) % yh);
  const long long n = i / ((long long)yw * yh);
  const long long plane = (long long)h * w;
  const float* p = img + n * c * plane + (long long)(row + crop) * w + (col + crop);
  float v;
  if (c == 3) {
    const float r = __fdiv_rn(quant_u8(p[0]), 255.f), g = __fdiv_rn(quant_u8(p[plane]), 255.f),
                b = __fdiv_rn(quant_u8(p[2 * plane]), 255.f);
    const double d = (((double)b * 24.966 + (double)g * 128.553) + (double)r * 65.481) + 16.0;
    v = (float)(d / 255.0) * 255.f;
  } else {
    v = __fdiv_rn(quant_u8(p[0]), 255.f) * 255.f;
  }
  y[i] = v;
}

// Scale-2 image: cv2.resize(y / 255., (w/2, h/2), INTER_LINEAR) * 255. of an even-sided image = the 2x2 cell mean,
// (((a00 + a01) + a10) + a11) * 0.25 in f32 on a = f32(y / 255).
__global__ __launch_bounds__(256) void niqe_half_kernel(const float* __restrict__ y, int yh, int yw, float* __restrict__ out,
                                                        long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int w2 = yw / 2, h2 = yh / 2;
  const int col = (int)(i % w2), row = (int)((i / w2) % h2);
  const long long n = i / ((long long)w2 * h2);
  const float* p = y + (n * yh + 2 * row) * yw + 2 * col;
  const float a00 = __fdiv_rn(p[0], 255.f), a01 = __fdiv_rn(p[1], 255.f), a10 = __fdiv_rn(p[yw], 255.f),
              a11 = __fdiv_rn(p[yw + 1], 255.f);
  out[i] = ((((a00 + a01) + a10) + a11) * 0.25f) * 255.f;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// One workgroup per B x B block of one image (blockIdx.x = block in the reference's order: block column outer, block row
// inner; blockIdx.y = image).  The (B+6)^2 halo tile of the H x W image is staged in LDS with the edge replicated at the
// IMAGE border (scipy mode='nearest'); each thread forms the MSCN of B*B/256 pixels, the block's MSCN then replaces the
// tile in LDS for the wrapped neighbour products (np.roll inside the block, products in f32).  Per field (MSCN and the four
// products) five float64 sums: n_neg, sum b^2 | b<0, n_pos, sum b^2 | b>0, sum |b|; zeros count in neither side.
template <int B>
__global__ __launch_bounds__(256) void niqe_moments_kernel(const float* __restrict__ img, int H, int W, NiqeWin win,
                                                           double* __restrict__ mom, float* __restrict__ mscn_out) {
  constexpr int T = B + 6, NPT = B * B / 256;
  static_assert(B * B % 256 == 0, "pixels per thread");
  __shared__ float tile[T * T];
  __shared__ double red[4][25];
  const int tid = threadIdx.x, n = blockIdx.y, nbh = H / B, nb = nbh * (W / B);
  const int blk = blockIdx.x, bw = blk / nbh, bh = blk % nbh;
  const float* src = img + (size_t)n * H * W;
  const int r0 = bh * B - 3, c0 = bw * B - 3;
  for (int i = tid; i < T * T; i += 256) {
    const int r = min(max(r0 + i / T, 0), H - 1), cc = min(max(c0 + i % T, 0), W - 1);
    tile[i] = src[(size_t)r * W + cc];
  }
  __syncthreads();
  float m[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int p = tid + 256 * k, i = p / B, j = p % B;
    double mu = 0.0, ex2 = 0.0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
      for (int b = 0; b < 7; ++b) {
        const float x = tile[(i + a) * T + j + b];
        const double t = win.w[a * 7 + b];
        mu += t * (double)x;
        ex2 += t * (double)(x * x);
      }
    const float muf = (float)mu, ex2f = (float)ex2;
    // f32 sqrt correctly rounded: v_sqrt_f32 (what sqrtf and __fsqrt_rn compile to) is not; the fp64 root rounded to f32 is
    const float sigma = (float)sqrt((double)fabsf(ex2f - muf * muf));
    m[k] = __fdiv_rn(tile[(i + 3) * T + j + 3] - muf, sigma + 1.f);
    if (mscn_out) mscn_out[((size_t)n * H + bh * B + i) * W + bw * B + j] = m[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NPT; ++k) tile[tid + 256 * k] = m[k];  // tile[i * B + j]: the block's MSCN
  __syncthreads();
  double acc[5][5];
#pragma unroll
  for (int f = 0; f < 5; ++f)
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[f][q] = 0.0;
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int p = tid + 256 * k, i = p / B, j = p % B;
    const int iu = (i + B - 1) % B, jl = (j + B - 1) % B, jr = (j + 1) % B;  // np.roll(block, s)[i][j] = block[i - s0][j - s1]
    const float b0 = m[k];
    const float v[5] = {b0, b0 * tile[i * B + jl], b0 * tile[iu * B + j], b0 * tile[iu * B + jl], b0 * tile[iu * B + jr]};
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const double d = (double)v[f], sq = d * d;
      if (v[f] < 0.f) {
        acc[f][0] += 1.0;
        acc[f][1] += sq;
      } else if (v[f] > 0.f) {
        acc[f][2] += 1.0;
        acc[f][3] += sq;
      }
      acc[f][4] += fabs(d);
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int f = 0; f < 5; ++f)
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const double s = wave_sum(acc[f][q]);
      if (lane == 0) red[wave][f * 5 + q] = s;
    }
  __syncthreads();
  if (tid < 25) mom[((size_t)n * nb + blk) * 25 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

unsigned nblk(long long n) { return (unsigned)((n + 255) / 256); }
}  // namespace

extern "C" size_t sr_niqe_workspace_bytes(int n, int yh, int yw) {
  if (n <= 0 || yh <= 0 || yw <= 0) return 0;
  return (size_t)n * (yh / 2) * (yw / 2) * sizeof(float);
}

extern "C" int sr_niqe_luma_f32(const float* img, int n, int c, int h, int w, int crop_border, float* y, int yh, int yw,
                                void* stream) {
  SR_CHECK_ARG(img && y && n > 0 && n < 65536 && (c == 1 || c == 3) && crop_border >= 0, "sr_niqe_luma_f32: bad argument");
  SR_CHECK_ARG(yh > 0 && yw > 0 && yh % kBlock == 0 && yw % kBlock == 0 && yh <= h - 2 * crop_border && yw <= w - 2 * crop_border,
               "sr_niqe_luma_f32: yh x yw (%d x %d) must be positive multiples of %d inside the %d x %d image less crop_border %d",
               yh, yw, kBlock, h, w, crop_border);
  const long long total = (long long)n * yh * yw;
  hipLaunchKernelGGL(niqe_luma_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, img, c, h, w, crop_border, y, yh, yw,
                     total);
  SR_CHECK_LAUNCH("niqe_luma");
  return SR_OK;
}

extern "C" int sr_niqe_moments_f32(const float* y, int n, int yh, int yw, int scale, const double* host_window, double* moments,
                                   float* mscn_out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(y && host_window && moments && n > 0 && n < 65536 && (scale == 1 || scale == 2), "sr_niqe_moments_f32: bad argument");
  SR_CHECK_ARG(yh > 0 && yw > 0 && yh % kBlock == 0 && yw % kBlock == 0, "sr_niqe_moments_f32: yh x yw (%d x %d) must be positive "
               "multiples of %d", yh, yw, kBlock);
  SR_CHECK_ARG(scale == 1 || (ws && ws_bytes >= sr_niqe_workspace_bytes(n, yh, yw)), "sr_niqe_moments_f32: workspace %zu B < %zu B",
               ws_bytes, sr_niqe_workspace_bytes(n, yh, yw));
  NiqeWin win;
  for (int a = 0; a < 7; ++a)
    for (int b = 0; b < 7; ++b) win.w[a * 7 + b] = host_window[(6 - a) * 7 + (6 - b)];
  const int nb = (yh / kBlock) * (yw / kBlock);
  if (scale == 1) {
    hipLaunchKernelGGL(niqe_moments_kernel<kBlock>, dim3(nb, n), dim3(256), 0, stream, y, yh, yw, win, moments, mscn_out);
  } else {
    const long long total = (long long)n * (yh / 2) * (yw / 2);
    hipLaunchKernelGGL(niqe_half_kernel, dim3(nblk(total)), dim3(256), 0, stream, y, yh, yw, (float*)ws, total);
    hipLaunchKernelGGL(niqe_moments_kernel<kBlock / 2>, dim3(nb, n), dim3(256), 0, stream, (const float*)ws, yh / 2, yw / 2, win,
                       moments, mscn_out);
  }
  SR_CHECK_LAUNCH("niqe_moments");
  return SR_OK;
}
