// RIDNet (basicsr/archs/ridnet_arch.py) on fp32 MFMA for gfx950: the convolutions no other kernel of the library computes,
// and the small passes around them (include/sr_hip_ridnet.h).
//
// Dilated 3x3 / 1x1 convolution, stride 1, pad d*(k-1)/2: the implicit GEMM of conv_f32.hip (D[cout][pixel] += W[cout][k] *
// X[k][pixel] on v_mfma_f32_32x32x2_f32, CB8 layout, LDS-DMA staging through buffer descriptors, double-buffered chunks of one
// 8-channel block, the same weight image and LDS bank swizzle), with two changes: the staged X tile carries a halo of d*(k-1)/2
// pixels ([TH + 2d][32 + 2d][8] for a 3x3) and tap (ty, tx) reads it d*ty rows and d*tx columns further on; and the epilogue
// can apply the activation after the residual adds.  A 1x1 conv is the one-tap instance (no halo), not a 3x3 of zero taps.
// Per chunk the MFMA work is that of the dense conv; what grows with d is the staged X tile (d = 4, TH = 8: 16 x 40 pixels
// against 10 x 34), i.e. LDS-DMA bytes per chunk.
//
// Weight gradient: the row-ring kernel of wgrad_f32.hip with a ring of 2 + d*(k-1) rows and X rows of 32 + d*(k-1) pixels;
// partial tiles go to a slab and through sr::wgrad_reduce (fixed order, no atomics).
//
// MeanShift ends (3 channels): elementwise mixes, and their weight gradients as per-workgroup partials + a fixed-order finish.
#include <algorithm>

#include "sr_internal.h"
#include "../../include/sr_hip_ridnet.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

struct ConvdParams {
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  const float* res1;
  const float* res2;
  const float* mask;
  float* pre;
  long long in_ns, out_ns, res1_ns, res2_ns, mask_ns, pre_ns;
  int cin_blocks, cout_blocks;
  int H, W;  // input = output size
  int tiles_x, tiles_y;
  int mask_cb0, mask_cb1, res_cb1;
  float slope, alpha, beta1, beta2, mask_slope;
  int accumulate, post;
};

// LDS-DMA of 16 bytes per lane through a buffer descriptor.  Kept in a __device__ function (wgrad_f32.hip): with the builtin in
// the kernel body itself, hipcc's host pass drops kernel stubs.
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, char* lds_dst) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
}

// One 32-column x (4*PT)-row x (32*COT)-cout tile per workgroup of 4 waves; KS x KS taps DIL apart.
template <int COT, int PT, int KS, int DIL>
__global__ __launch_bounds__(256) void convd_f32_kernel(const ConvdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = 4, HALO = (KS - 1) * DIL;
  constexpr int TH = NW * PT, XROW = 32 + HALO, XPIX = (TH + HALO) * XROW;
  constexpr int XBYTES = ((XPIX * 32 + 1023) / 1024) * 1024;
  constexpr int NXU = XBYTES / 1024, NWU = KS * KS * COT;
  constexpr int WBYTES = NWU * 1024, STAGE = XBYTES + WBYTES;
  constexpr int NXR = (NXU + NW - 1) / NW, NWR = (NWU + NW - 1) / NW;
  constexpr int W_CHUNK = WBYTES / 4;  // floats of one channel block's weight image

  int t;
  {  // XCD-aware tile order (conv_f32.hip)
    const int nwg = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  }
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int n = t / p.tiles_y;
  const int cog = blockIdx.y;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int x0 = tx * 32, y0 = ty * TH;
  const int HW = p.H * p.W;
  const float* in_n = p.in + (long long)n * p.in_ns;
  const float* wg = p.w + (size_t)cog * p.cin_blocks * W_CHUNK;

  // per-lane byte offsets of the X pieces this wave moves (beyond the buffer = zero padding), computed once per tile
  unsigned xvo[NXR];
#pragma unroll
  for (int r = 0; r < NXR; ++r) {
    const int u = r * NW + wave;
    const int q = u * 64 + lane;
    const int pix = q >> 1, half = q & 1;
    const int row = pix / XROW, col = pix - row * XROW;
    const int gy = y0 - HALO / 2 + row, gx = x0 - HALO / 2 + col;
    const bool valid = pix < XPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
    const int hsw = half ^ ((col >> 3) & 1);  // LDS bank swizzle of conv_f32.hip
    xvo[r] = valid ? (unsigned)((gy * p.W + gx) * 8 + hsw * 4) * 4u : 0xfffffff0u;
  }
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)in_n, 0, (unsigned)((long long)p.cin_blocks * HW * 8 * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)wg, 0, (unsigned)((long long)p.cin_blocks * W_CHUNK * 4), 0x00020000);
  const unsigned wvo = (lane ^ ((lane >> 4) & 1)) * 16;
  auto stage = [&](int buf, int cb) {
    char* xs = smem + buf * STAGE;
    char* ws = xs + XBYTES;
    const unsigned xso = (unsigned)cb * (unsigned)HW * 32u, wso = (unsigned)cb * (unsigned)W_CHUNK * 4u;
#pragma unroll
    for (int r = 0; r < NXR; ++r) {
      const int u = r * NW + wave;
      if (u < NXU)
        blds16(x_rs, xvo[r], xso, xs + u * 1024);
    }
#pragma unroll
    for (int r = 0; r < NWR; ++r) {
      const int u = r * NW + wave;  // unit = tap * COT + cout sub-tile
      if (u < NWU)
        blds16(w_rs, wvo, wso + (unsigned)(u * 256) * 4u, ws + u * 1024);
    }
  };

  f32x16 acc[COT][PT];
#pragma unroll
  for (int a = 0; a < COT; ++a)
#pragma unroll
    for (int b = 0; b < PT; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int xrow0 = (wave * PT * XROW + j) * 32;
  int xlane[KS];
#pragma unroll
  for (int dx = 0; dx < KS; ++dx) xlane[dx] = xrow0 + dx * DIL * 32 + ((h ^ (((j + dx * DIL) >> 3) & 1)) * 16);
  const int wlane = j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  auto compute = [&](int buf) {
    const char* xb = smem + buf * STAGE;
    const char* ws = smem + buf * STAGE + XBYTES + wlane;
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) {
#pragma unroll
      for (int dx = 0; dx < KS; ++dx) {
        const int tap = dy * KS + dx;
        f32x4 a[COT], b[PT];
#pragma unroll
        for (int c = 0; c < COT; ++c) a[c] = *(const f32x4*)(ws + (tap * COT + c) * 1024);
#pragma unroll
        for (int r = 0; r < PT; ++r) b[r] = *(const f32x4*)(xb + xlane[dx] + (r + dy * DIL) * XROW * 32);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int c = 0; c < COT; ++c)
#pragma unroll
            for (int r = 0; r < PT; ++r)
              acc[c][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][s], b[r][s], acc[c][r], 0, 0, 0);
      }
    }
  };

  const int nchunk = p.cin_blocks;
  stage(0, 0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    if (c + 1 < nchunk) stage((c + 1) & 1, c + 1);
    compute(c & 1);
    __syncthreads();
  }

  // epilogue (conv_f32.hip's, in its operation order when post == 0)
  const int x = x0 + j;
  if (x >= p.W) return;
#pragma unroll
  for (int r = 0; r < PT; ++r) {
    const int y = y0 + wave * PT + r;
    if (y >= p.H) continue;
    const long long pixoff = (long long)y * p.W + x;
#pragma unroll
    for (int c = 0; c < COT; ++c) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = (cog * COT + c) * 4 + g;
        if (cb >= p.cout_blocks) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[c][r][g * 4 + e];
        const long long off = (cb * (long long)HW + pixoff) * 8 + h * 4;
        float* o = p.out + (long long)n * p.out_ns + off;
        if (p.bias) v += *(const f32x4*)(p.bias + cb * 8 + h * 4);
        if (p.post) {
          v *= p.alpha;
          if (p.res1 && cb < p.res_cb1) v += p.beta1 * *(const f32x4*)(p.res1 + (long long)n * p.res1_ns + off);
          if (p.res2 && cb < p.res_cb1) v += p.beta2 * *(const f32x4*)(p.res2 + (long long)n * p.res2_ns + off);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
          v *= p.alpha;
          if (p.pre) *(f32x4*)(p.pre + (long long)n * p.pre_ns + off) = v;
          if (p.res1 && cb < p.res_cb1) v += p.beta1 * *(const f32x4*)(p.res1 + (long long)n * p.res1_ns + off);
          if (p.res2 && cb < p.res_cb1) v += p.beta2 * *(const f32x4*)(p.res2 + (long long)n * p.res2_ns + off);
        }
        if (p.accumulate) v += *(const f32x4*)o;
        if (p.mask && cb >= p.mask_cb0 && cb < p.mask_cb1) {
          const f32x4 m = *(const f32x4*)(p.mask + (long long)n * p.mask_ns + ((cb - p.mask_cb0) * (long long)HW + pixoff) * 8 + h * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : v[e] * p.mask_slope;
        }
        *(f32x4*)o = v;
      }
    }
  }
}

template <int COT, int PT, int KS, int DIL>
constexpr int convd_lds_bytes() {
  return 2 * ((((4 * PT + (KS - 1) * DIL) * (32 + (KS - 1) * DIL) * 32 + 1023) / 1024) * 1024 + KS * KS * COT * 1024);
}

template <int COT, int PT, int KS, int DIL>
int convd_launch(const ConvdParams& p, int n, int groups, const sr_convd_desc* d, hipStream_t stream) {
  constexpr int lds = convd_lds_bytes<COT, PT, KS, DIL>();
  auto kern = convd_f32_kernel<COT, PT, KS, DIL>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, lds)) return rc;
  const bool prof = sr::prof_on();
  if (prof) {
    const sr_conv3x3_desc* b = &d->base;
    sr_launch_record r = {};
    r.kernel_id = KS == 3 ? 81 : 82;
    r.cin = b->cin_real > 0 ? b->cin_real : b->cin_pad;
    r.cout = b->cout;
    r.n = n;
    r.h = p.H;
    r.w = p.W;
    const double px = (double)n * p.H * p.W;
    r.flops = 2.0 * KS * KS * r.cin * r.cout * px;
    double fl = px * (r.cin + r.cout);
    if (b->res1) fl += px * r.cout;
    if (b->res2) fl += px * r.cout;
    if (b->accumulate) fl += px * r.cout;
    if (b->mask_src) fl += px * b->mask_cbn * 8;
    if (d->out_pre) fl += px * r.cout;
    r.bytes = 4.0 * fl;
    sr::prof_begin(stream, r);
  }
  hipLaunchKernelGGL(kern, dim3(p.tiles_x * p.tiles_y * n, groups), dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("convd_f32 launch");
  return SR_OK;
}

template <int KS, int DIL>
int convd_dispatch(ConvdParams p, int n, int gc, int groups, const sr_convd_desc* d, hipStream_t stream) {
  // 8-row tiles; 4-row tiles when the launch would not cover the chip once (as sr_conv3x3_f32)
  p.tiles_y = sr::cdiv(p.H, 8);
  const bool small = (long long)p.tiles_x * p.tiles_y * n * groups < 256 && p.H > 4;
  if (small) p.tiles_y = sr::cdiv(p.H, 4);
  if (gc == 64) return small ? convd_launch<2, 1, KS, DIL>(p, n, groups, d, stream) : convd_launch<2, 2, KS, DIL>(p, n, groups, d, stream);
  return small ? convd_launch<1, 1, KS, DIL>(p, n, groups, d, stream) : convd_launch<1, 2, KS, DIL>(p, n, groups, d, stream);
}

// ------------------------------------------------------------------------------------------------------- weight packing
// sr::conv_group_couts (conv_f32.hip), usable in the pack kernel: couts per weight-image group
__host__ __device__ __forceinline__ int group_couts(int cout) { return (((cout + 31) / 32 * 32) % 64 == 0) ? 64 : 32; }

// wp[g][cb][tap][co % gc][c8] (mode 0), the layout of sr_conv3x3_pack_f32 with ks*ks taps; mode 1: output channel = ci,
// input channel = co, tap flipped.
__global__ void convk_pack_kernel(const float* __restrict__ w, int cout, int cin, int ks, int mode, float* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nt = ks * ks;
  if (i >= cout * cin * nt) return;
  const int tap = i % nt, ci = (i / nt) % cin, co = i / (nt * cin);
  const float val = w[i];
  if (mode == 0) {
    const int gc = group_couts(cout), cbs = (cin + 7) / 8;
    wp[((((long long)(co / gc) * cbs + (ci >> 3)) * nt + tap) * gc + co % gc) * 8 + (ci & 7)] = val;
  } else {
    const int gc = group_couts((cin + 7) / 8 * 8), cbs = (cout + 7) / 8;
    wp[((((long long)(ci / gc) * cbs + (co >> 3)) * nt + (nt - 1 - tap)) * gc + ci % gc) * 8 + (co & 7)] = val;
  }
}

__global__ void convk_pack_bias_kernel(const float* __restrict__ b, int cout, int cpad, float* __restrict__ bp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cpad) bp[i] = i < cout ? b[i] : 0.f;
}

}  // namespace

extern "C" size_t sr_convk_packed_weight_floats(int cout, int cin, int ksize, int mode) {
  if (cout <= 0 || cin <= 0 || (ksize != 1 && ksize != 3)) return 0;
  const int oc = mode == 0 ? cout : (cin + 7) / 8 * 8, ic = mode == 0 ? (cin + 7) / 8 * 8 : (cout + 7) / 8 * 8;
  return (size_t)((oc + 31) / 32 * 32) * ic * ksize * ksize;
}

extern "C" int sr_convk_pack_f32(const float* weight, const float* bias, int cout, int cin, int ksize, int mode, float* wpacked,
                                 float* bpacked, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(weight && wpacked && cout > 0 && cin > 0, "sr_convk_pack_f32: bad argument");
  SR_CHECK_ARG(ksize == 1 || ksize == 3, "sr_convk_pack_f32: ksize must be 1 or 3 (got %d)", ksize);
  SR_CHECK_ARG(mode == 0 || mode == 1, "sr_convk_pack_f32: mode must be 0 or 1");
  const size_t wfloats = sr_convk_packed_weight_floats(cout, cin, ksize, mode);
  if (hipMemsetAsync(wpacked, 0, wfloats * sizeof(float), stream) != hipSuccess) {
    sr::set_error("sr_convk_pack_f32: memset failed");
    return SR_ELAUNCH;
  }
  const int total = cout * cin * ksize * ksize;
  hipLaunchKernelGGL(convk_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, weight, cout, cin, ksize, mode, wpacked);
  SR_CHECK_LAUNCH("convk_pack");
  if (bias && bpacked && mode == 0) {
    const int cp = (cout + 31) / 32 * 32;
    hipLaunchKernelGGL(convk_pack_bias_kernel, dim3((cp + 255) / 256), dim3(256), 0, stream, bias, cout, cp, bpacked);
    SR_CHECK_LAUNCH("convk_pack_bias");
  }
  return SR_OK;
}

extern "C" int sr_convd_f32(const sr_convd_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_convd_f32: null descriptor");
  const sr_conv3x3_desc& b = d->base;
  SR_CHECK_ARG(b.in && b.wpacked && b.out, "sr_convd_f32: null in/wpacked/out");
  SR_CHECK_ARG((d->ksize == 3 && d->dilation >= 1 && d->dilation <= 4) || (d->ksize == 1 && d->dilation == 1),
               "sr_convd_f32: ksize %d / dilation %d not supported (3 with 1..4, or 1 with 1)", d->ksize, d->dilation);
  SR_CHECK_ARG(b.cin_pad > 0 && b.cin_pad % 8 == 0, "sr_convd_f32: cin_pad=%d must be a positive multiple of 8", b.cin_pad);
  SR_CHECK_ARG(b.cout > 0 && b.n > 0 && b.in_h > 0 && b.in_w > 0, "sr_convd_f32: bad shape");
  SR_CHECK_ARG(!b.upsample && !b.out_nchw && !b.out_h && !b.out_w && !b.s2_channels && !b.out_unshuffle2 && !b.res1_u2 &&
                   !b.res1_keep_sign,
               "sr_convd_f32: upsample / out_nchw / out_h / out_w and the bf16 options are not supported");
  SR_CHECK_ARG(!(d->post_act && d->out_pre), "sr_convd_f32: out_pre needs post_act = 0");
  SR_CHECK_ARG(((uintptr_t)b.in | (uintptr_t)b.wpacked | (uintptr_t)b.out | (uintptr_t)b.res1 | (uintptr_t)b.res2 |
                (uintptr_t)b.mask_src | (uintptr_t)b.bpacked | (uintptr_t)d->out_pre) % 16 == 0,
               "sr_convd_f32: pointers must be 16-byte aligned");
  const int cin_blocks = b.cin_pad / 8, cout_blocks = (b.cout + 7) / 8;
  const long long blocks = std::max(cin_blocks, cout_blocks);
  SR_CHECK_ARG((long long)b.in_h * b.in_w * 8 * blocks * 4 < (1ll << 32), "sr_convd_f32: image too large for 32-bit offsets");
  ConvdParams p = {};
  p.in = b.in;
  p.w = b.wpacked;
  p.bias = b.bpacked;
  p.out = b.out;
  p.res1 = b.res1;
  p.res2 = b.res2;
  p.mask = b.mask_src;
  p.pre = d->out_pre;
  p.in_ns = b.in_img_stride;
  p.out_ns = b.out_img_stride;
  p.res1_ns = b.res1_img_stride;
  p.res2_ns = b.res2_img_stride;
  p.mask_ns = b.mask_img_stride;
  p.pre_ns = d->out_pre_img_stride;
  p.cin_blocks = cin_blocks;
  p.cout_blocks = cout_blocks;
  p.H = b.in_h;
  p.W = b.in_w;
  p.tiles_x = sr::cdiv(p.W, 32);
  p.mask_cb0 = b.mask_cb0;
  p.mask_cb1 = b.mask_cb0 + b.mask_cbn;
  p.res_cb1 = b.res_cbn > 0 ? b.res_cbn : (1 << 30);
  p.slope = b.act_slope;
  p.alpha = b.alpha;
  p.beta1 = b.beta1;
  p.beta2 = b.beta2;
  p.mask_slope = b.mask_slope;
  p.accumulate = b.accumulate;
  p.post = d->post_act;
  const int gc = group_couts(b.cout);
  const int groups = ((b.cout + 31) / 32 * 32) / gc;
  SR_CHECK_ARG((long long)p.tiles_x * sr::cdiv(p.H, 4) * b.n < (1ll << 31), "sr_convd_f32: grid too large");
  if (d->ksize == 1) return convd_dispatch<1, 1>(p, b.n, gc, groups, d, stream);
  switch (d->dilation) {
    case 1: return convd_dispatch<3, 1>(p, b.n, gc, groups, d, stream);
    case 2: return convd_dispatch<3, 2>(p, b.n, gc, groups, d, stream);
    case 3: return convd_dispatch<3, 3>(p, b.n, gc, groups, d, stream);
    default: return convd_dispatch<3, 4>(p, b.n, gc, groups, d, stream);
  }
}

// ------------------------------------------------------------------------------------------------------ weight gradient
namespace {

struct WgraddParams {
  const float* x;   // forward source, CB8
  const float* dy;  // gradient at the conv's pre-activation output, CB8
  float* slab;      // [group][split][pair][tap][1024]
  float* bslab;     // [group row][split][CT][32] or null
  long long x_ns, dy_ns;
  int H, W;
  int cin_blocks, cout_blocks;
  int gi;           // cin groups per cout-group row
  int strips, rows_per_wg, row_splits;
};


// wgrad_f32_body (wgrad_f32.hip) with R = 1 (the 4/P waves of a pair split the 16 pixel-pair k-steps of a row), KT x KT taps
// DIL apart: X rows of 32 + HALO pixels in a ring of 2 + HALO rows, dY rows in a ring of 2.
template <int CT, int IT, int KT, int DIL>
__global__ __launch_bounds__(256) void wgradd_f32_kernel(const WgraddParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int P = CT * IT, KS = 4 / P;
  constexpr int SN = 16 / KS;
  constexpr int HALO = (KT - 1) * DIL;
  constexpr int XCH = 32 * IT, YCH = 32 * CT;
  constexpr int XPIX = 32 + HALO;
  constexpr int XPIECES = XPIX * (XCH / 4);
  constexpr int XUNITS = (XPIECES + 63) / 64;
  constexpr int XROWB = XUNITS * 1024;
  constexpr int YUNITS = (32 * (YCH / 4)) / 64;
  constexpr int YROWB = YUNITS * 1024;
  constexpr int NXR = 2 + HALO, NYR = 2;
  constexpr int XRING = NXR * XROWB;
  constexpr int UNITS_PER_STEP = XUNITS + YUNITS;
  constexpr int UPW = (UNITS_PER_STEP + 3) / 4;
  constexpr int NT = KT * KT;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int ct = wave / (IT * KS), it = (wave / KS) % IT, ks = wave % KS;
  const int by = blockIdx.y, bx = blockIdx.x;
  const int grow = by / p.gi, gcol = by - grow * p.gi;
  const int cout_tile0 = grow * CT, cin_tile0 = gcol * IT;

  int t = bx;
  const int rs = t % p.row_splits;
  t /= p.row_splits;
  const int strip = t % p.strips;
  const int n = t / p.strips;
  const int x0 = strip * 32;
  const int y_begin = rs * p.rows_per_wg;
  const int y_end = min(y_begin + p.rows_per_wg, p.H);

  const float* xn = p.x + (long long)n * p.x_ns;
  const float* dyn = p.dy + (long long)n * p.dy_ns;
  const long long plane = (long long)p.H * p.W * 8;
  char* xring = smem;
  char* yring = smem + XRING;

  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)xn, 0, (unsigned)((long long)p.cin_blocks * plane * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t y_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)dyn, 0, (unsigned)((long long)p.cout_blocks * plane * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t null_rs = __builtin_amdgcn_make_buffer_rsrc((void*)xn, 0, 0, 0x00020000);
  unsigned lane_off[UPW];
#pragma unroll
  for (int uu = 0; uu < UPW; ++uu) {
    const int v = uu * 4 + wave;
    unsigned off = 0xfffffff0u;
    if (v < XUNITS) {
      const int q = v * 64 + lane;
      const int pix = q / (XCH / 4), c4 = q % (XCH / 4);
      const int cb = cin_tile0 * 4 + (c4 >> 1);
      const int gx = x0 - HALO / 2 + pix;
      if (q < XPIECES && gx >= 0 && gx < p.W && cb < p.cin_blocks) off = (unsigned)((cb * plane + (long long)gx * 8 + (c4 & 1) * 4) * 4);
    } else if (v < UNITS_PER_STEP) {
      const int q = (v - XUNITS) * 64 + lane;
      const int pix = q / (YCH / 4), c4 = q % (YCH / 4);
      const int cb = cout_tile0 * 4 + (c4 >> 1);
      const int gx = x0 + pix;
      if (gx < p.W && cb < p.cout_blocks) off = (unsigned)((cb * plane + (long long)gx * 8 + (c4 & 1) * 4) * 4);
    }
    lane_off[uu] = off;
  }
  // X tap-row u (virtual source row u - HALO/2) goes to ring slot u % NXR; dY row y to slot y % NYR
  auto stage = [&](int ux, int yy, bool with_dy) {
#pragma unroll
    for (int uu = 0; uu < UPW; ++uu) {
      const int v = uu * 4 + wave;
      if (v >= UNITS_PER_STEP) break;
      if (v < XUNITS) {
        const int sy = ux - HALO / 2;
        const bool ok = sy >= 0 && sy < p.H;
        blds16(ok ? x_rs : null_rs, lane_off[uu], ok ? (unsigned)sy * (unsigned)p.W * 32u : 0u, xring + (ux % NXR) * XROWB + v * 1024);
      } else if (with_dy) {
        const bool ok = yy < p.H;
        blds16(ok ? y_rs : null_rs, lane_off[uu], ok ? (unsigned)yy * (unsigned)p.W * 32u : 0u,
               yring + (yy % NYR) * YROWB + (v - XUNITS) * 1024);
      }
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
  float bsum = 0.f;

  const int a_lane = (h * YCH + ct * 32 + j) * 4;
  const int b_lane = (h * XCH + it * 32 + j) * 4;

  // Invariant at the top of step y: X tap-rows [y, y + HALO + 1) and dY row y are in LDS; during step y, tap-row y + HALO + 1
  // and dY row y + 1 arrive.  Live: NXR = HALO + 2 tap-rows, NYR = 2 dY rows.
  stage(y_begin, y_begin, true);
  for (int u0 = y_begin + 1; u0 <= y_begin + HALO; ++u0) stage(u0, 0, false);
  __syncthreads();
  for (int y = y_begin; y < y_end; ++y) {
    stage(y + HALO + 1, y + 1, true);
    const int s0 = ks * SN;
    const char* ya = yring + (y % NYR) * YROWB + a_lane + s0 * 2 * YCH * 4;
    const char* xb[KT];
#pragma unroll
    for (int dy = 0; dy < KT; ++dy) xb[dy] = xring + ((y + dy * DIL) % NXR) * XROWB + b_lane + s0 * 2 * XCH * 4;
    float a_cur, b_cur[KT][KT];
    a_cur = *(const float*)ya;
#pragma unroll
    for (int dy = 0; dy < KT; ++dy)
#pragma unroll
      for (int dx = 0; dx < KT; ++dx) b_cur[dy][dx] = *(const float*)(xb[dy] + dx * DIL * XCH * 4);
#pragma unroll
    for (int s = 0; s < SN; ++s) {
      float a_nxt = 0.f, b_nxt[KT][KT];
      if (s + 1 < SN) {
        a_nxt = *(const float*)(ya + (s + 1) * 2 * YCH * 4);
#pragma unroll
        for (int dy = 0; dy < KT; ++dy)
#pragma unroll
          for (int dx = 0; dx < KT; ++dx) b_nxt[dy][dx] = *(const float*)(xb[dy] + ((s + 1) * 2 + dx * DIL) * XCH * 4);
      }
      __builtin_amdgcn_sched_barrier(0);
      bsum += a_cur;
#pragma unroll
      for (int dy = 0; dy < KT; ++dy)
#pragma unroll
        for (int dx = 0; dx < KT; ++dx)
          acc[dy * KT + dx] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur, b_cur[dy][dx], acc[dy * KT + dx], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (s + 1 < SN) {
        a_cur = a_nxt;
#pragma unroll
        for (int dy = 0; dy < KT; ++dy)
#pragma unroll
          for (int dx = 0; dx < KT; ++dx) b_cur[dy][dx] = b_nxt[dy][dx];
      }
    }
    __syncthreads();
  }

  const int pair = ct * IT + it;
  const long long nsplit = (long long)gridDim.x * KS;
  const long long split = (long long)bx * KS + ks;
  float* dst = p.slab + (((by * nsplit + split) * P + pair) * NT) * 1024 + lane * 4;
#pragma unroll
  for (int tap = 0; tap < NT; ++tap)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[tap][g * 4 + e];
      *(f32x4*)(dst + tap * 1024 + g * 256) = v;
    }
  if (p.bslab && it == 0 && gcol == 0) {
    bsum += __shfl_xor(bsum, 32);
    if (h == 0) p.bslab[((grow * nsplit + split) * CT + ct) * 32 + j] = bsum;
  }
}

template <int CT, int IT, int KT, int DIL>
constexpr int wgradd_lds_bytes() {
  constexpr int XUNITS = ((32 + (KT - 1) * DIL) * (32 * IT / 4) + 63) / 64, YUNITS = 4 * CT;
  return (2 + (KT - 1) * DIL) * XUNITS * 1024 + 2 * YUNITS * 1024;
}

// Launch shape of one weight gradient: tile pair (CT, IT), group grid, rows per workgroup.  Shared by the size query and the call.
struct WgraddPlan {
  int CT, IT, grows, gi, strips, rows, row_splits;
  long long nwg, splits;
  size_t slab_floats, bslab_floats;
};
constexpr size_t kPartFloats = (size_t)64 * 4 * 9 * 1024, kBpartFloats = 4096;  // sr::wgrad_reduce's partial buffers

WgraddPlan wgradd_plan(int n, int h, int w, int cout, int cin_pad, int ks, int dil) {
  WgraddPlan q = {};
  const int cts = sr::cdiv(cout, 32), its = sr::cdiv(cin_pad, 32);
  const bool wide = ks == 1 || dil <= 2;  // 2x2 tile pairs while the ring fits two workgroups per CU
  if (cts % 2 == 0 && its % 2 == 0 && wide) {
    q.CT = 2, q.IT = 2;
  } else if (cts % 2 == 0 && !wide) {
    q.CT = 2, q.IT = 1;
  } else {
    q.CT = 1, q.IT = 1;
  }
  q.grows = cts / q.CT;
  q.gi = its / q.IT;
  q.strips = sr::cdiv(w, 32);
  const long long strips_total = (long long)n * q.strips;
  const int groups = q.grows * q.gi;
  int rows = h;
  while (rows > 4 && strips_total * sr::cdiv(h, rows) * groups < 512) rows = (rows + 1) / 2;
  q.rows = rows;
  q.row_splits = sr::cdiv(h, rows);
  q.nwg = strips_total * q.row_splits;
  q.splits = q.nwg * (4 / (q.CT * q.IT));
  q.slab_floats = (size_t)groups * q.splits * q.CT * q.IT * ks * ks * 1024;
  q.bslab_floats = (size_t)q.grows * q.splits * q.CT * 32;
  return q;
}

template <int CT, int IT, int KT, int DIL>
int wgradd_launch(const WgraddParams& p, const WgraddPlan& q, const sr_conv3x3_wgrad_desc* d, hipStream_t stream) {
  constexpr int lds = wgradd_lds_bytes<CT, IT, KT, DIL>();
  auto kern = wgradd_f32_kernel<CT, IT, KT, DIL>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, lds)) return rc;
  const bool prof = sr::prof_on();
  if (prof) {
    sr_launch_record r = {};
    r.kernel_id = KT == 3 ? 83 : 84;
    r.cin = d->cin;
    r.cout = d->cout;
    r.n = d->n;
    r.h = p.H;
    r.w = p.W;
    const double px = (double)d->n * p.H * p.W;
    r.flops = 2.0 * KT * KT * d->cin * d->cout * px;
    r.bytes = 4.0 * px * (d->cin_pad + d->cout);
    sr::prof_begin(stream, r);
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)q.nwg, (unsigned)(q.grows * q.gi)), dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("wgradd_f32 launch");
  return SR_OK;
}

template <int KT, int DIL>
int wgradd_variant(const WgraddParams& p, const WgraddPlan& q, const sr_conv3x3_wgrad_desc* d, hipStream_t stream) {
  if (q.CT == 2 && q.IT == 2) return wgradd_launch<2, 2, KT, DIL>(p, q, d, stream);
  if (q.CT == 2) return wgradd_launch<2, 1, KT, DIL>(p, q, d, stream);
  return wgradd_launch<1, 1, KT, DIL>(p, q, d, stream);
}

size_t wgradd_bytes(const WgraddPlan& q) {
  return sr::align_up(q.slab_floats * 4, 256) + sr::align_up(q.bslab_floats * 4, 256) + sr::align_up(kPartFloats * 4, 256) +
         sr::align_up(kBpartFloats * 4, 256);
}

}  // namespace

extern "C" size_t sr_convd_wgrad_slab_bytes(int n, int h, int w, int cout, int cin, int ksize, int dilation) {
  if (n <= 0 || h <= 0 || w <= 0 || cout <= 0 || cin <= 0) return 0;
  if (!((ksize == 3 && dilation >= 1 && dilation <= 4) || (ksize == 1 && dilation == 1))) return 0;
  return wgradd_bytes(wgradd_plan(n, h, w, cout, (cin + 7) / 8 * 8, ksize, dilation));
}

extern "C" int sr_convd_wgrad_f32(const sr_convd_wgrad_desc* dd, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(dd != nullptr, "sr_convd_wgrad_f32: null descriptor");
  const sr_conv3x3_wgrad_desc* d = &dd->base;
  SR_CHECK_ARG(d->x && d->dy && d->dweight && d->slab, "sr_convd_wgrad_f32: null argument");
  SR_CHECK_ARG((dd->ksize == 3 && dd->dilation >= 1 && dd->dilation <= 4) || (dd->ksize == 1 && dd->dilation == 1),
               "sr_convd_wgrad_f32: ksize %d / dilation %d not supported", dd->ksize, dd->dilation);
  SR_CHECK_ARG(d->cout > 0 && d->cin > 0 && d->n > 0 && d->in_h > 0 && d->in_w > 0, "sr_convd_wgrad_f32: bad shape");
  SR_CHECK_ARG(!d->upsample && d->first_seg == d->cin && d->seg == 0 && d->cin_pad == (d->cin + 7) / 8 * 8,
               "sr_convd_wgrad_f32: dense cin only (upsample 0, first_seg = cin, seg 0, cin_pad = roundup8(cin))");
  SR_CHECK_ARG((long long)d->in_h * d->in_w * 4 * 4 * ((d->cout > d->cin_pad ? d->cout : d->cin_pad) + 7) < (1ll << 32),
               "sr_convd_wgrad_f32: image too large for 32-bit buffer offsets");
  SR_CHECK_ARG(((uintptr_t)d->x | (uintptr_t)d->dy) % 16 == 0, "sr_convd_wgrad_f32: pointers must be 16-byte aligned");
  SR_CHECK_ARG((uintptr_t)d->slab % 256 == 0, "sr_convd_wgrad_f32: slab must be 256-byte aligned");
  const WgraddPlan q = wgradd_plan(d->n, d->in_h, d->in_w, d->cout, d->cin_pad, dd->ksize, dd->dilation);
  const size_t need = wgradd_bytes(q);
  if (d->slab_bytes < need) {
    sr::set_error("sr_convd_wgrad_f32: slab %zu B too small (need %zu B)", d->slab_bytes, need);
    return SR_ENOSPACE;
  }
  char* base = (char*)d->slab;
  float* slab = (float*)base;
  base += sr::align_up(q.slab_floats * 4, 256);
  float* bslab = (float*)base;
  base += sr::align_up(q.bslab_floats * 4, 256);
  float* part = (float*)base;
  base += sr::align_up(kPartFloats * 4, 256);
  float* bpart = (float*)base;

  WgraddParams p = {};
  p.x = d->x;
  p.dy = d->dy;
  p.slab = slab;
  p.bslab = d->dbias ? bslab : nullptr;
  p.x_ns = d->x_img_stride;
  p.dy_ns = d->dy_img_stride;
  p.H = d->in_h;
  p.W = d->in_w;
  p.cin_blocks = d->cin_pad / 8;
  p.cout_blocks = (d->cout + 7) / 8;
  p.gi = q.gi;
  p.strips = q.strips;
  p.rows_per_wg = q.rows;
  p.row_splits = q.row_splits;
  int rc;
  if (dd->ksize == 1) {
    rc = wgradd_variant<1, 1>(p, q, d, stream);
  } else {
    switch (dd->dilation) {
      case 1: rc = wgradd_variant<3, 1>(p, q, d, stream); break;
      case 2: rc = wgradd_variant<3, 2>(p, q, d, stream); break;
      case 3: rc = wgradd_variant<3, 3>(p, q, d, stream); break;
      default: rc = wgradd_variant<3, 4>(p, q, d, stream); break;
    }
  }
  if (rc) return rc;
  sr::WgradReduce r = {};
  r.slab = slab;
  r.bslab = p.bslab;
  r.part = part;
  r.bpart = bpart;
  r.splits = q.splits;
  r.groups = q.grows * q.gi;
  r.gi = q.gi;
  r.P = q.CT * q.IT;
  r.IT = q.IT;
  r.CT = q.CT;
  r.ntap = dd->ksize * dd->ksize;
  r.ks = dd->ksize;
  r.kdim = dd->ksize;
  r.t_mul = 1;
  r.cout = d->cout;
  r.cin = d->cin;
  r.first_seg = d->cin;
  r.seg = 0;
  r.seg_pad = 8;
  r.scale = d->scale;
  r.accumulate = d->accumulate;
  r.dw = d->dweight;
  r.db = d->dbias;
  return sr::wgrad_reduce(r, stream);
}

// --------------------------------------------------------------------------------------------------------- MeanShift ends
namespace {

constexpr int kMeanThreads = 256;
constexpr int kMeanPixels = 4096;  // pixels per workgroup of the backward partials: 16 per thread

__global__ __launch_bounds__(256) void sub_mean_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ b, float* __restrict__ s, long long s_ns, long long HW,
                                                       long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long n = i / HW, px = i - n * HW;
  const float* xi = x + n * 3 * HW + px;
  const float x0 = xi[0], x1 = xi[HW], x2 = xi[2 * HW];
  f32x4 lo, hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) lo[c] = w[c * 3] * x0 + w[c * 3 + 1] * x1 + w[c * 3 + 2] * x2 + b[c];
  lo[3] = 0.f;
  f32x4* o = (f32x4*)(s + n * s_ns + px * 8);
  o[0] = lo;
  o[1] = hi;
}

__global__ __launch_bounds__(256) void add_mean_kernel(const float* __restrict__ x, const float* __restrict__ t, long long t_ns,
                                                       const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ y,
                                                       long long HW, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long n = i / HW, px = i - n * HW;
  const f32x4 tv = *(const f32x4*)(t + n * t_ns + px * 8);
  const float* xi = x + n * 3 * HW + px;
  float* yi = y + n * 3 * HW + px;
#pragma unroll
  for (int c = 0; c < 3; ++c) yi[c * HW] = xi[c * HW] + (w[c * 3] * tv[0] + w[c * 3 + 1] * tv[1] + w[c * 3 + 2] * tv[2] + b[c]);
}

// One workgroup per (image, band of kMeanPixels pixels): the 12 sums dW[c][k] = sum g[c] a[k], db[c] = sum g[c] over the band,
// combined by a fixed butterfly within each wave and in wave order, into part[n][band][12]; and the elementwise adjoint:
//   SUB: a = x (NCHW), g CB8;  dx (NCHW, optional) = W^T g (+ dres)
//   ADD: a = t (CB8),  g NCHW; dt (CB8, 8 channels) = W^T g
template <bool SUB>
__global__ __launch_bounds__(256) void mean_bwd_partial_kernel(const float* __restrict__ a, long long a_ns, const float* __restrict__ g,
                                                               long long g_ns, const float* __restrict__ w, float* __restrict__ da,
                                                               long long da_ns, const float* __restrict__ dres, long long HW, int bands,
                                                               float* __restrict__ part) {
  __shared__ float red[kMeanThreads / 64][12];
  const int band = blockIdx.x, n = blockIdx.y;
  const long long p0 = (long long)band * kMeanPixels, p1 = min(HW, p0 + kMeanPixels);
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
  float wt[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wt[k] = w[k];
  for (long long px = p0 + threadIdx.x; px < p1; px += kMeanThreads) {
    float av[3], gv[3];
    if (SUB) {
      const float* xi = a + n * a_ns + px;
      av[0] = xi[0], av[1] = xi[HW], av[2] = xi[2 * HW];
      const f32x4 gg = *(const f32x4*)(g + n * g_ns + px * 8);
      gv[0] = gg[0], gv[1] = gg[1], gv[2] = gg[2];
    } else {
      const f32x4 tv = *(const f32x4*)(a + n * a_ns + px * 8);
      av[0] = tv[0], av[1] = tv[1], av[2] = tv[2];
      const float* gi = g + n * g_ns + px;
      gv[0] = gi[0], gv[1] = gi[HW], gv[2] = gi[2 * HW];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[c * 3 + k] += gv[c] * av[k];
      acc[9 + c] += gv[c];
    }
    if (da) {
      float dv[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) dv[k] = wt[k] * gv[0] + wt[3 + k] * gv[1] + wt[6 + k] * gv[2];
      if (SUB) {
        float* o = da + n * da_ns + px;
        const float* r = dres ? dres + n * da_ns + px : nullptr;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k * HW] = r ? dv[k] + r[k * HW] : dv[k];
      } else {
        f32x4* o = (f32x4*)(da + n * da_ns + px * 8);
        o[0] = f32x4{dv[0], dv[1], dv[2], 0.f};
        o[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 12; ++k) red[wave][k] = acc[k];
  __syncthreads();
  if (part && threadIdx.x < 12) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int v = 1; v < kMeanThreads / 64; ++v) s += red[v][threadIdx.x];
    part[((long long)n * bands + band) * 12 + threadIdx.x] = s;
  }
}

// dW / db: one thread per output, the (image, band) partials summed in order.
__global__ void mean_bwd_finish_kernel(const float* __restrict__ part, long long nparts, float* __restrict__ dw, float* __restrict__ db,
                                       int accumulate) {
  const int k = threadIdx.x;
  if (k >= 12) return;
  float s = 0.f;
  for (long long i = 0; i < nparts; ++i) s += part[i * 12 + k];
  float* o = k < 9 ? (dw ? dw + k : nullptr) : (db ? db + (k - 9) : nullptr);
  if (o) *o = accumulate ? *o + s : s;
}

long long mean_bands(long long hw) { return (hw + kMeanPixels - 1) / kMeanPixels; }

void prof_small(hipStream_t stream, int id, int c, int n, int h, int w, double flops, double bytes) {
  sr_launch_record r = {};
  r.kernel_id = id;
  r.cin = c;
  r.cout = c;
  r.n = n;
  r.h = h;
  r.w = w;
  r.flops = flops;
  r.bytes = bytes;
  sr::prof_begin(stream, r);
}

template <bool SUB>
int mean_bwd(const float* a, long long a_ns, const float* g, long long g_ns, const float* w, float* dw, float* db, int accumulate,
             float* da, long long da_ns, const float* dres, int n, int h, int w_, void* workspace, size_t workspace_bytes,
             hipStream_t stream, const char* who) {
  SR_CHECK_ARG(a && g && w && n > 0 && h > 0 && w_ > 0, "%s: bad argument", who);
  SR_CHECK_ARG(workspace || (!dw && !db), "%s: null workspace", who);
  const long long HW = (long long)h * w_, bands = mean_bands(HW);
  SR_CHECK_ARG(bands < 65536 && n < 65536, "%s: image too large", who);
  if (dw || db) {
    if (workspace_bytes < sr_ridnet_mean_workspace_bytes(n, h, w_)) {
      sr::set_error("%s: workspace %zu B too small", who, workspace_bytes);
      return SR_ENOSPACE;
    }
  }
  float* part = (dw || db) ? (float*)workspace : nullptr;
  const bool prof = sr::prof_on();
  if (prof) prof_small(stream, 87, 3, n, h, w_, 2.0 * 12 * n * HW, 4.0 * n * HW * (6 + (da ? 3 : 0)));
  hipLaunchKernelGGL(mean_bwd_partial_kernel<SUB>, dim3((unsigned)bands, (unsigned)n), dim3(kMeanThreads), 0, stream, a, a_ns, g, g_ns,
                     w, da, da_ns, dres, HW, (int)bands, part);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("mean_bwd_partial launch");
  if (dw || db) {
    if (prof) prof_small(stream, 88, 3, n, h, w_, (double)n * bands * 12, 4.0 * n * bands * 12);
    hipLaunchKernelGGL(mean_bwd_finish_kernel, dim3(1), dim3(64), 0, stream, (const float*)part, (long long)n * bands, dw, db, accumulate);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("mean_bwd_finish launch");
  }
  return SR_OK;
}

// out = u * s[n][c] (SCALE) or out = mask > 0 ? g : slope * g, one 16-byte half pixel per thread.
template <bool SCALE>
__global__ __launch_bounds__(256) void cb8_stream_kernel(const float* __restrict__ a, long long a_ns, const float* __restrict__ b,
                                                         long long b_ns, float slope, float* __restrict__ out, long long out_ns, int cbn,
                                                         long long HW, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int half = (int)(i & 1);
  long long r = i >> 1;
  const long long px = r % HW;
  r /= HW;
  const int cb = (int)(r % cbn);
  const long long n = r / cbn;
  const long long off = ((long long)cb * HW + px) * 8 + half * 4;
  f32x4 v = *(const f32x4*)(a + n * a_ns + off);
  if (SCALE) {
    v *= *(const f32x4*)(b + n * (long long)cbn * 8 + cb * 8 + half * 4);
  } else {
    const f32x4 m = *(const f32x4*)(b + n * b_ns + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : v[e] * slope;
  }
  *(f32x4*)(out + n * out_ns + off) = v;
}

}  // namespace

extern "C" size_t sr_ridnet_mean_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return sr::align_up((size_t)n * mean_bands((long long)h * w) * 12 * sizeof(float), 256);
}

extern "C" int sr_ridnet_sub_mean_f32(const float* x, const float* w, const float* b, float* s, int64_t s_img_stride, int n, int h,
                                      int w_, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && w && b && s && n > 0 && h > 0 && w_ > 0, "sr_ridnet_sub_mean_f32: bad argument");
  SR_CHECK_ARG((uintptr_t)s % 16 == 0 && s_img_stride % 4 == 0, "sr_ridnet_sub_mean_f32: s must be 16-byte aligned");
  const long long HW = (long long)h * w_, total = n * HW;
  const bool prof = sr::prof_on();
  if (prof) prof_small(stream, 85, 3, n, h, w_, 2.0 * 9 * total, 4.0 * total * (3 + 8));
  hipLaunchKernelGGL(sub_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, w, b, s, (long long)s_img_stride,
                     HW, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sub_mean launch");
  return SR_OK;
}

extern "C" int sr_ridnet_add_mean_f32(const float* x, const float* t, int64_t t_img_stride, const float* w, const float* b, float* y,
                                      int n, int h, int w_, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && t && w && b && y && n > 0 && h > 0 && w_ > 0, "sr_ridnet_add_mean_f32: bad argument");
  SR_CHECK_ARG((uintptr_t)t % 16 == 0 && t_img_stride % 4 == 0, "sr_ridnet_add_mean_f32: t must be 16-byte aligned");
  const long long HW = (long long)h * w_, total = n * HW;
  const bool prof = sr::prof_on();
  if (prof) prof_small(stream, 86, 3, n, h, w_, 2.0 * 9 * total, 4.0 * total * (3 + 4 + 3));
  hipLaunchKernelGGL(add_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, t, (long long)t_img_stride, w, b, y,
                     HW, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("add_mean launch");
  return SR_OK;
}

extern "C" int sr_ridnet_sub_mean_bwd_f32(const float* x, const float* g, int64_t g_img_stride, const float* w, float* dw, float* db,
                                          int accumulate, float* dx, const float* dx_res, int n, int h, int w_, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  SR_CHECK_ARG((uintptr_t)g % 16 == 0 && g_img_stride % 4 == 0, "sr_ridnet_sub_mean_bwd_f32: g must be 16-byte aligned");
  return mean_bwd<true>(x, 3ll * h * w_, g, g_img_stride, w, dw, db, accumulate, dx, 3ll * h * w_, dx_res, n, h, w_, workspace,
                        workspace_bytes, (hipStream_t)stream, "sr_ridnet_sub_mean_bwd_f32");
}

extern "C" int sr_ridnet_add_mean_bwd_f32(const float* g, const float* t, int64_t t_img_stride, const float* w, float* dw, float* db,
                                          int accumulate, float* dt, int64_t dt_img_stride, int n, int h, int w_, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  SR_CHECK_ARG(((uintptr_t)t | (uintptr_t)dt) % 16 == 0 && t_img_stride % 4 == 0 && dt_img_stride % 4 == 0,
               "sr_ridnet_add_mean_bwd_f32: t / dt must be 16-byte aligned");
  return mean_bwd<false>(t, t_img_stride, g, 3ll * h * w_, w, dw, db, accumulate, dt, dt_img_stride, nullptr, n, h, w_, workspace,
                         workspace_bytes, (hipStream_t)stream, "sr_ridnet_add_mean_bwd_f32");
}

extern "C" int sr_ca_scale_f32(const float* u, int64_t u_img_stride, const float* s, float* out, int64_t out_img_stride, int n, int nf,
                               int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(u && s && out && n > 0 && nf > 0 && nf % 8 == 0 && h > 0 && w > 0, "sr_ca_scale_f32: bad argument");
  SR_CHECK_ARG(((uintptr_t)u | (uintptr_t)out | (uintptr_t)s) % 16 == 0, "sr_ca_scale_f32: pointers must be 16-byte aligned");
  const long long HW = (long long)h * w, total = (long long)n * (nf / 8) * HW * 2;
  const bool prof = sr::prof_on();
  if (prof) prof_small(stream, 89, nf, n, h, w, (double)n * nf * HW, 8.0 * n * nf * HW);
  hipLaunchKernelGGL(cb8_stream_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, u, (long long)u_img_stride, s,
                     0ll, 0.f, out, (long long)out_img_stride, nf / 8, HW, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("ca_scale launch");
  return SR_OK;
}

extern "C" int sr_cb8_relu_mask_f32(const float* g, int64_t g_img_stride, const float* mask, int64_t mask_img_stride, float slope,
                                    float* out, int64_t out_img_stride, int n, int cbn, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(g && mask && out && n > 0 && cbn > 0 && h > 0 && w > 0, "sr_cb8_relu_mask_f32: bad argument");
  SR_CHECK_ARG(((uintptr_t)g | (uintptr_t)out | (uintptr_t)mask) % 16 == 0, "sr_cb8_relu_mask_f32: pointers must be 16-byte aligned");
  const long long HW = (long long)h * w, total = (long long)n * cbn * HW * 2;
  const bool prof = sr::prof_on();
  if (prof) prof_small(stream, 90, cbn * 8, n, h, w, (double)n * cbn * 8 * HW, 12.0 * n * cbn * 8 * HW);
  hipLaunchKernelGGL(cb8_stream_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, g, (long long)g_img_stride,
                     mask, (long long)mask_img_stride, slope, out, (long long)out_img_stride, cbn, HW, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("relu_mask launch");
  return SR_OK;
}
