// GFPGANv1OCR's StyleGAN2 decoder (stylegan2_ocr_arch.py / gfpganv1_ocr_arch.py of the reference) on fp32 for gfx950,
// inference only (include/sr_hip_gfpgan.h).
//
// Modulated 3x3 conv: the implicit GEMM of ridnet_ops.hip's dilated conv at dilation 1 (D[cout][pixel] += W[cout][k] * X[k][pixel]
// on v_mfma_f32_32x32x2_f32, CB8 layout, LDS-DMA staging through buffer descriptors, double-buffered chunks of one 8-channel
// block, the same weight image and LDS bank swizzle) on the SHARED weight image: the source already holds x * s[n] (its producer
// wrote it) and the epilogue applies d[n][co], the noise, the FusedLeakyReLU, the SFT and the next layer's s[n].
// Upsampling conv: the same GEMM, one output parity of the stride-2 transposed conv per workgroup (4, 2, 2 or 1 taps of the
// 3x3 weight image), into the raw (2h+1) x (2w+1) map; a streaming pass applies the 4x4 blur and the tail.
// ToRGB, the style coefficients and NormStyleCode are small streaming / reduction kernels.
#include <algorithm>

#include "sr_internal.h"
#include "../../include/sr_hip_gfpgan.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// ----------------------------------------------------------------------------------------------------------- the tail
struct Tail {
  const float* demod;
  const float* bias;
  const float* noise;
  const float* sft_s;
  const float* sft_t;
  const float* s_next;
  long long noise_ns, sfts_ns, sftt_ns;
  int cout, sft_cb0;
  float noise_w, slope, alpha;
};

// The tail of include/sr_hip_gfpgan.h on channels cb * 8 + h * 4 + [0, 4) of sample n at pixel `pix` of an HW-pixel map.
__device__ __forceinline__ f32x4 apply_tail(f32x4 v, const Tail& t, int n, int cb, int h, long long pix, long long HW) {
  const int c0 = cb * 8 + h * 4;
  v *= *(const f32x4*)(t.demod + (long long)n * t.cout + c0);
  if (t.noise) {
    const float z = t.noise_w * t.noise[n * t.noise_ns + pix];
    v += z;
  }
  v += *(const f32x4*)(t.bias + c0);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * t.slope;
  v *= t.alpha;
  if (t.sft_s && cb >= t.sft_cb0) {
    const long long o = ((long long)(cb - t.sft_cb0) * HW + pix) * 8 + h * 4;
    v = v * *(const f32x4*)(t.sft_s + n * t.sfts_ns + o);
    v = v + *(const f32x4*)(t.sft_t + n * t.sftt_ns + o);
  }
  if (t.s_next) v *= *(const f32x4*)(t.s_next + (long long)n * t.cout + c0);
  return v;
}

Tail make_tail(const sr_gfpgan_tail* t, const float* bias, int cout, float slope, float alpha) {
  Tail r = {};
  r.demod = t->demod;
  r.bias = bias;
  r.noise = t->noise;
  r.noise_ns = t->noise_img_stride;
  r.noise_w = t->noise_strength;
  r.sft_s = t->sft_scale;
  r.sft_t = t->sft_shift;
  r.sfts_ns = t->sft_scale_img_stride;
  r.sftt_ns = t->sft_shift_img_stride;
  r.sft_cb0 = t->sft_c0 / 8;
  r.s_next = t->s_next;
  r.cout = cout;
  r.slope = slope;
  r.alpha = alpha;
  return r;
}

int check_tail(const sr_gfpgan_tail* t, int cout, const char* who) {
  SR_CHECK_ARG(t && t->demod, "%s: the tail needs demod", who);
  SR_CHECK_ARG(!t->sft_scale == !t->sft_shift, "%s: sft_scale and sft_shift go together", who);
  SR_CHECK_ARG(!t->sft_scale || (t->sft_c0 >= 0 && t->sft_c0 % 8 == 0 && t->sft_c0 < cout),
               "%s: sft_c0=%d must be a multiple of 8 below cout", who, t->sft_c0);
  SR_CHECK_ARG(((uintptr_t)t->demod | (uintptr_t)t->sft_scale | (uintptr_t)t->sft_shift | (uintptr_t)t->s_next) % 16 == 0 &&
                   t->sft_scale_img_stride % 4 == 0 && t->sft_shift_img_stride % 4 == 0,
               "%s: tail tensors must be 16-byte aligned", who);
  return SR_OK;
}

// --------------------------------------------------------------------------------------------- modulated convolutions
struct ModParams {
  const float* in;
  const float* w;
  float* out;
  long long in_ns, out_ns;
  int cin_blocks, cout_blocks;
  int H, W;  // source size
  int tiles_x, tiles_y;
  Tail tail;
};

// LDS-DMA of 16 bytes per lane through a buffer descriptor (in a __device__ function: with the builtin in the kernel body,
// hipcc's host pass drops kernel stubs).
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, char* lds_dst) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
}

__device__ __forceinline__ int xcd_tile() {  // XCD-aware tile order (conv_f32.hip)
  const int nwg = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// One 32-column x (4*PT)-row x (32*COT)-cout tile per workgroup of 4 waves, taps (ky, kx) of the 3x3 weight image.  UP = 0: the
// stride-1 3x3 conv, tap (ky, kx) at source offset (ky - 1, kx - 1), the tail as epilogue.  UP = 1: output parity (PY, PX) of the
// stride-2 transposed conv on its (H + 1 - PY) x (W + 1 - PX) grid; grid point (i, j) takes tap ky = 1 at source row i (PY = 1)
// or ky = 2 at row i - 1 and ky = 0 at row i (PY = 0), likewise kx, and is stored raw at (2i + PY, 2j + PX) of the
// (2H + 1) x (2W + 1) map.  Staged X tile: rows y0 - 1 .. y0 + TH (- 1 for UP), columns x0 - 1 .. x0 + 32 (- 1 for UP).
template <int COT, int PT, int UP, int PY, int PX>
__device__ __forceinline__ void modconv_body(const ModParams& p, char* smem, int t, int cog) {
  constexpr int NW = 4, TH = NW * PT;
  constexpr int HALO = UP ? 1 : 2;
  constexpr int XROW = 32 + HALO, XPIX = (TH + HALO) * XROW;
  constexpr int XBYTES = ((XPIX * 32 + 1023) / 1024) * 1024;
  constexpr int NTY = UP ? (PY ? 1 : 2) : 3, NTX = UP ? (PX ? 1 : 2) : 3;
  constexpr int NXU = XBYTES / 1024, NWU = NTY * NTX * COT;
  constexpr int WBYTES = NWU * 1024, STAGE = XBYTES + WBYTES;
  constexpr int NXR = (NXU + NW - 1) / NW, NWR = (NWU + NW - 1) / NW;
  constexpr int W_CHUNK = 9 * COT * 256;  // floats of one channel block's weight image (all nine taps)

  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int n = t / p.tiles_y;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int x0 = tx * 32, y0 = ty * TH;
  const int HW = p.H * p.W;
  const float* in_n = p.in + (long long)n * p.in_ns;
  const float* wg = p.w + (size_t)cog * p.cin_blocks * W_CHUNK;

  unsigned xvo[NXR];
#pragma unroll
  for (int r = 0; r < NXR; ++r) {
    const int u = r * NW + wave;
    const int q = u * 64 + lane;
    const int pix = q >> 1, half = q & 1;
    const int row = pix / XROW, col = pix - row * XROW;
    const int gy = y0 - 1 + row, gx = x0 - 1 + col;
    const bool valid = pix < XPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
    const int hsw = half ^ ((col >> 3) & 1);
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
      if (u < NXU) blds16(x_rs, xvo[r], xso, xs + u * 1024);
    }
#pragma unroll
    for (int r = 0; r < NWR; ++r) {
      const int u = r * NW + wave;  // unit = local tap * COT + cout sub-tile
      if (u < NWU) {
        const int lt = u / COT, c = u - lt * COT;
        const int a = lt / NTX, b = lt - a * NTX;
        const int ky = UP ? (PY ? 1 : (a ? 0 : 2)) : a, kx = UP ? (PX ? 1 : (b ? 0 : 2)) : b;
        blds16(w_rs, wvo, wso + (unsigned)(((ky * 3 + kx) * COT + c) * 256) * 4u, ws + u * 1024);
      }
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
  int xlane[HALO + 1];
#pragma unroll
  for (int dx = 0; dx <= HALO; ++dx) xlane[dx] = xrow0 + dx * 32 + ((h ^ (((j + dx) >> 3) & 1)) * 16);
  const int wlane = j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  auto compute = [&](int buf) {
    const char* xb = smem + buf * STAGE;
    const char* ws = smem + buf * STAGE + XBYTES + wlane;
#pragma unroll
    for (int a = 0; a < NTY; ++a) {
#pragma unroll
      for (int b = 0; b < NTX; ++b) {
        const int lt = a * NTX + b;
        const int ro = UP ? (PY ? 1 : a) : a, cof = UP ? (PX ? 1 : b) : b;  // staged row / column offset of the tap
        f32x4 av[COT], bv[PT];
#pragma unroll
        for (int c = 0; c < COT; ++c) av[c] = *(const f32x4*)(ws + (lt * COT + c) * 1024);
#pragma unroll
        for (int r = 0; r < PT; ++r) bv[r] = *(const f32x4*)(xb + xlane[cof] + (r + ro) * XROW * 32);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int c = 0; c < COT; ++c)
#pragma unroll
            for (int r = 0; r < PT; ++r) acc[c][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c][s], bv[r][s], acc[c][r], 0, 0, 0);
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

  const int x = x0 + j;
  const int GH = UP ? p.H + 1 - PY : p.H, GW = UP ? p.W + 1 - PX : p.W;  // output grid of this parity
  if (x >= GW) return;
  const int OW = UP ? 2 * p.W + 1 : p.W;
  const long long OHW = UP ? (long long)(2 * p.H + 1) * OW : (long long)HW;
#pragma unroll
  for (int r = 0; r < PT; ++r) {
    const int y = y0 + wave * PT + r;
    if (y >= GH) continue;
    const long long pixoff = UP ? (long long)(2 * y + PY) * OW + (2 * x + PX) : (long long)y * OW + x;
#pragma unroll
    for (int c = 0; c < COT; ++c) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = (cog * COT + c) * 4 + g;
        if (cb >= p.cout_blocks) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[c][r][g * 4 + e];
        float* o = p.out + (long long)n * p.out_ns + (cb * OHW + pixoff) * 8 + h * 4;
        *(f32x4*)o = UP ? v : apply_tail(v, p.tail, n, cb, h, pixoff, OHW);
      }
    }
  }
}

template <int COT, int PT>
__global__ __launch_bounds__(256) void gfp_modconv_kernel(const ModParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  modconv_body<COT, PT, 0, 0, 0>(p, smem, xcd_tile(), blockIdx.y);
}

// blockIdx.y = cout group * 4 + parity; each workgroup runs one parity (a uniform branch).
template <int COT, int PT>
__global__ __launch_bounds__(256) void gfp_upconv_kernel(const ModParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int par = blockIdx.y & 3, cog = blockIdx.y >> 2;
  const int t = xcd_tile();
  if (par == 0)
    modconv_body<COT, PT, 1, 0, 0>(p, smem, t, cog);
  else if (par == 1)
    modconv_body<COT, PT, 1, 0, 1>(p, smem, t, cog);
  else if (par == 2)
    modconv_body<COT, PT, 1, 1, 0>(p, smem, t, cog);
  else
    modconv_body<COT, PT, 1, 1, 1>(p, smem, t, cog);
}

template <int COT, int PT, int UP>
constexpr int modconv_lds_bytes() {
  constexpr int HALO = UP ? 1 : 2, NT = UP ? 4 : 9;
  return 2 * ((((4 * PT + HALO) * (32 + HALO) * 32 + 1023) / 1024) * 1024 + NT * COT * 1024);
}

__host__ __device__ __forceinline__ int group_couts(int cout) { return (((cout + 31) / 32 * 32) % 64 == 0) ? 64 : 32; }

template <int COT, int PT, int UP>
int modconv_launch(const ModParams& p, int n, int groups, const sr_gfpgan_modconv_desc* d, hipStream_t stream) {
  constexpr int lds = modconv_lds_bytes<COT, PT, UP>();
  auto kern = UP ? gfp_upconv_kernel<COT, PT> : gfp_modconv_kernel<COT, PT>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, lds)) return rc;
  const bool prof = sr::prof_on();
  if (prof) {
    const sr_conv3x3_desc* b = &d->base;
    const int cin = b->cin_real > 0 ? b->cin_real : b->cin_pad;
    const double px = (double)n * p.H * p.W;
    const double opx = UP ? (double)n * (2 * p.H + 1) * (2 * p.W + 1) : px;
    sr::prof_rec(stream, UP ? 93 : 92, cin, b->cout, n, p.H, p.W, 18.0 * cin * b->cout * px, 4.0 * (px * cin + opx * b->cout));
  }
  hipLaunchKernelGGL(kern, dim3(p.tiles_x * p.tiles_y * n, groups * (UP ? 4 : 1)), dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(UP ? "gfpgan upconv launch" : "gfpgan modconv launch");
  return SR_OK;
}

template <int UP>
int modconv_common(const sr_gfpgan_modconv_desc* d, hipStream_t stream, const char* who) {
  SR_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  const sr_conv3x3_desc& b = d->base;
  SR_CHECK_ARG(b.in && b.wpacked && b.out && (UP || b.bpacked), "%s: null in/wpacked/out/bpacked", who);
  SR_CHECK_ARG(b.cin_pad > 0 && b.cin_pad % 8 == 0, "%s: cin_pad=%d must be a positive multiple of 8", who, b.cin_pad);
  SR_CHECK_ARG(b.cout > 0 && b.cout % 8 == 0 && b.n > 0 && b.in_h > 0 && b.in_w > 0, "%s: bad shape (cout must be a multiple of 8)",
               who);
  SR_CHECK_ARG(!b.upsample && !b.out_nchw && !b.out_h && !b.out_w && !b.res1 && !b.res2 && !b.accumulate && !b.mask_src &&
                   !b.s2_channels && !b.out_unshuffle2 && !b.res1_u2 && !b.res1_keep_sign,
               "%s: only in / wpacked / bpacked / out / act_slope / alpha are honoured", who);
  SR_CHECK_ARG(((uintptr_t)b.in | (uintptr_t)b.wpacked | (uintptr_t)b.out | (uintptr_t)b.bpacked) % 16 == 0 && b.in_img_stride % 4 == 0 &&
                   b.out_img_stride % 4 == 0,
               "%s: pointers must be 16-byte aligned", who);
  if (!UP)
    if (int rc = check_tail(&d->tail, b.cout, who)) return rc;
  const int cin_blocks = b.cin_pad / 8, cout_blocks = b.cout / 8;
  const long long oh = UP ? 2ll * b.in_h + 1 : b.in_h, ow = UP ? 2ll * b.in_w + 1 : b.in_w;
  SR_CHECK_ARG((long long)b.in_h * b.in_w * 8 * cin_blocks * 4 < (1ll << 32) && oh * ow * 8 * cout_blocks < (1ll << 31),
               "%s: image too large for 32-bit offsets", who);
  ModParams p = {};
  p.in = b.in;
  p.w = b.wpacked;
  p.out = b.out;
  p.in_ns = b.in_img_stride;
  p.out_ns = b.out_img_stride;
  p.cin_blocks = cin_blocks;
  p.cout_blocks = cout_blocks;
  p.H = b.in_h;
  p.W = b.in_w;
  if (!UP) p.tail = make_tail(&d->tail, b.bpacked, b.cout, b.act_slope, b.alpha);
  const int GH = UP ? p.H + 1 : p.H, GW = UP ? p.W + 1 : p.W;
  p.tiles_x = sr::cdiv(GW, 32);
  const int gc = group_couts(b.cout);
  const int groups = ((b.cout + 31) / 32 * 32) / gc;
  SR_CHECK_ARG((long long)p.tiles_x * sr::cdiv(GH, 4) * b.n < (1ll << 31), "%s: grid too large", who);
  // 8-row tiles; 4-row tiles when the launch would not cover the chip once (as sr_convd_f32)
  p.tiles_y = sr::cdiv(GH, 8);
  const bool small = (long long)p.tiles_x * p.tiles_y * b.n * groups * (UP ? 4 : 1) < 256 && GH > 4;
  if (small) p.tiles_y = sr::cdiv(GH, 4);
  if (gc == 64)
    return small ? modconv_launch<2, 1, UP>(p, b.n, groups, d, stream) : modconv_launch<2, 2, UP>(p, b.n, groups, d, stream);
  return small ? modconv_launch<1, 1, UP>(p, b.n, groups, d, stream) : modconv_launch<1, 2, UP>(p, b.n, groups, d, stream);
}

// ------------------------------------------------------------------------------------------------ blur + tail (upconv)
struct BlurParams {
  const float* t;
  float* out;
  long long t_ns, out_ns, total;
  int cbn, H, W;  // source size of the upconv: t is (2H + 1) x (2W + 1), out 2H x 2W
  Tail tail;
};

// out[y][x] = sum_{a,b} k[a] k[b] t[y + a - 1][x + b - 1] (zero outside), k = [1, 3, 3, 1] / 8 * 2, then the tail.
__global__ __launch_bounds__(256) void gfp_blur_up_kernel(const BlurParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int half = (int)(i & 1);
  const int WO = 2 * p.W, HO = 2 * p.H, WT = WO + 1, HT = HO + 1;
  long long r = i >> 1;
  const int x = (int)(r % WO);
  r /= WO;
  const int y = (int)(r % HO);
  r /= HO;
  const int cb = (int)(r % p.cbn);
  const int n = (int)(r / p.cbn);
  const float k[4] = {0.25f, 0.75f, 0.75f, 0.25f};
  const float* tb = p.t + n * p.t_ns + (long long)cb * HT * WT * 8 + half * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = y + a - 1;
    if (row < 0 || row >= HT) continue;
    f32x4 rs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = x + b - 1;
      if (col < 0 || col >= WT) continue;
      rs += k[b] * *(const f32x4*)(tb + ((long long)row * WT + col) * 8);
    }
    acc += k[a] * rs;
  }
  const long long pix = (long long)y * WO + x, OHW = (long long)HO * WO;
  *(f32x4*)(p.out + n * p.out_ns + ((long long)cb * OHW + pix) * 8 + half * 4) = apply_tail(acc, p.tail, n, cb, half, pix, OHW);
}

// ------------------------------------------------------------------------------------------------------------ ToRGB
struct RgbParams {
  const float* x;
  const float* w;
  const float* s;
  const float* bias;
  const float* skip;
  float* y;
  float* xn;
  const float* sn;
  long long x_ns, xn_ns;
  int C, H, W;
  float wscale;
};

// One thread per pixel of one image (blockIdx.y): the per-sample 3 x C weights (and s_next) in LDS.
__global__ __launch_bounds__(256) void gfp_torgb_kernel(const RgbParams p) {
  __shared__ float wn[3 * 512];
  __shared__ float sn[512];
  const int n = blockIdx.y;
  for (int i = threadIdx.x; i < 3 * p.C; i += 256) wn[i] = p.wscale * p.w[i] * p.s[(long long)n * p.C + i % p.C];
  if (p.xn)
    for (int i = threadIdx.x; i < p.C; i += 256) sn[i] = p.sn[(long long)n * p.C + i];
  __syncthreads();
  const long long HW = (long long)p.H * p.W;
  const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  const float* xb = p.x + n * p.x_ns + px * 8;
  for (int cb = 0; cb < p.C / 8; ++cb) {
    const f32x4 lo = *(const f32x4*)(xb + cb * HW * 8), hi = *(const f32x4*)(xb + cb * HW * 8 + 4);
    const float* w0 = wn + cb * 8;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a0 += w0[e] * lo[e];
      a1 += w0[p.C + e] * lo[e];
      a2 += w0[2 * p.C + e] * lo[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a0 += w0[4 + e] * hi[e];
      a1 += w0[p.C + 4 + e] * hi[e];
      a2 += w0[2 * p.C + 4 + e] * hi[e];
    }
    if (p.xn) {
      float* o = p.xn + n * p.xn_ns + (cb * HW + px) * 8;
      const float* s8 = sn + cb * 8;
      *(f32x4*)o = lo * f32x4{s8[0], s8[1], s8[2], s8[3]};
      *(f32x4*)(o + 4) = hi * f32x4{s8[4], s8[5], s8[6], s8[7]};
    }
  }
  float v[3] = {a0 + p.bias[0], a1 + p.bias[1], a2 + p.bias[2]};
  if (p.skip) {
    // upfirdn2d(skip, up 2, pad (2, 1)) with k = [1, 3, 3, 1] / 8 * 2 per axis: out[2t] = k0 skip[t-1] + k2 skip[t],
    // out[2t + 1] = k1 skip[t] + k3 skip[t+1], zero outside
    const int yy = (int)(px / p.W), xx = (int)(px - (long long)yy * p.W);
    const int h2 = p.H / 2, w2 = p.W / 2;
    const int ty = yy >> 1, tx = xx >> 1;
    const int ry0 = (yy & 1) ? ty : ty - 1, rx0 = (xx & 1) ? tx : tx - 1;
    const float ky[2] = {(yy & 1) ? 0.75f : 0.25f, (yy & 1) ? 0.25f : 0.75f};
    const float kx[2] = {(xx & 1) ? 0.75f : 0.25f, (xx & 1) ? 0.25f : 0.75f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* sk = p.skip + ((long long)n * 3 + c) * h2 * w2;
      float u = 0.f;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int ry = ry0 + a;
        if (ry < 0 || ry >= h2) continue;
        float rs = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int rx = rx0 + b;
          if (rx < 0 || rx >= w2) continue;
          rs += kx[b] * sk[(long long)ry * w2 + rx];
        }
        u += ky[a] * rs;
      }
      v[c] += u;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) p.y[((long long)n * 3 + c) * HW + px] = v[c];
}

// ------------------------------------------------------------------------------------------------ style coefficients
struct StyleLayerK {
  const float* A;
  const float* b;
  const float* q;
  float* s;
  float* d;
  int cin, cout, k;
  float wscale;
};

struct StyleParams {
  const float* lat;
  long long lat_ns, lat_rs;
  int nsf;
  float lin_scale;
  StyleLayerK L[SR_GFPGAN_MAX_LAYERS];
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One workgroup per (layer, sample): s = A latent / sqrt(nsf) + b, one output per wave step (lanes over the input, a fixed
// butterfly), then d from Q and s^2.
__global__ __launch_bounds__(256) void gfp_style_kernel(const StyleParams p) {
  __shared__ float lat[1024];
  __shared__ float s2[512];
  const StyleLayerK L = p.L[blockIdx.x];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lr = p.lat + n * p.lat_ns + L.k * p.lat_rs;
  for (int j = tid; j < p.nsf; j += 256) lat[j] = lr[j];
  __syncthreads();
  for (int ci = wave; ci < L.cin; ci += 4) {
    const float* a = L.A + (long long)ci * p.nsf;
    float acc = 0.f;
    for (int j = lane; j < p.nsf; j += 64) acc += a[j] * lat[j];
    acc = wave_sum(acc);
    const float s = acc * p.lin_scale + L.b[ci];
    if (lane == 0) {
      L.s[(long long)n * L.cin + ci] = s;
      s2[ci] = s * s;
    }
  }
  if (!L.q) return;
  __syncthreads();
  const float c2 = L.wscale * L.wscale;
  for (int co = wave; co < L.cout; co += 4) {
    const float* q = L.q + (long long)co * L.cin;
    float acc = 0.f;
    for (int ci = lane; ci < L.cin; ci += 64) acc += q[ci] * s2[ci];
    acc = wave_sum(acc);
    if (lane == 0) L.d[(long long)n * L.cout + co] = L.wscale / sqrtf(c2 * acc + 1e-8f);
  }
}

// NormStyleCode, one workgroup per row.
__global__ __launch_bounds__(256) void gfp_norm_kernel(const float* x, float* y, int nsf) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* xr = x + (long long)n * nsf;
  float acc = 0.f;
  for (int j = tid; j < nsf; j += 256) acc += xr[j] * xr[j];
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  const float m = (red[0] + red[1] + red[2] + red[3]) / (float)nsf;
  const float r = 1.f / sqrtf(m + 1e-8f);
  for (int j = tid; j < nsf; j += 256) y[(long long)n * nsf + j] = xr[j] * r;
}

}  // namespace

extern "C" int sr_gfpgan_modconv_f32(const sr_gfpgan_modconv_desc* d, void* stream) {
  return modconv_common<0>(d, (hipStream_t)stream, "sr_gfpgan_modconv_f32");
}

extern "C" int sr_gfpgan_upconv_f32(const sr_gfpgan_modconv_desc* d, void* stream) {
  return modconv_common<1>(d, (hipStream_t)stream, "sr_gfpgan_upconv_f32");
}

extern "C" int sr_gfpgan_blur_up_f32(const float* t, int64_t t_img_stride, float* out, int64_t out_img_stride, const float* bias,
                                     float act_slope, float alpha, const sr_gfpgan_tail* tail, int n, int cout, int h, int w,
                                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "sr_gfpgan_blur_up_f32";
  SR_CHECK_ARG(t && out && bias && n > 0 && cout > 0 && cout % 8 == 0 && h > 0 && w > 0, "%s: bad argument", who);
  SR_CHECK_ARG(((uintptr_t)t | (uintptr_t)out | (uintptr_t)bias) % 16 == 0 && t_img_stride % 4 == 0 && out_img_stride % 4 == 0,
               "%s: pointers must be 16-byte aligned", who);
  if (int rc = check_tail(tail, cout, who)) return rc;
  SR_CHECK_ARG((2ll * h + 1) * (2ll * w + 1) * cout < (1ll << 31), "%s: image too large", who);
  BlurParams p = {};
  p.t = t;
  p.out = out;
  p.t_ns = t_img_stride;
  p.out_ns = out_img_stride;
  p.cbn = cout / 8;
  p.H = h;
  p.W = w;
  p.total = (long long)n * p.cbn * 4ll * h * w * 2;
  p.tail = make_tail(tail, bias, cout, act_slope, alpha);
  const bool prof = sr::prof_on();
  const double opx = 4.0 * n * h * w;
  if (prof) sr::prof_rec(stream, 94, cout, cout, n, 2 * h, 2 * w, 32.0 * opx * cout, 4.0 * opx * cout * (2 + (tail->sft_scale ? 2 : 0)));
  hipLaunchKernelGGL(gfp_blur_up_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("gfpgan blur_up launch");
  return SR_OK;
}

extern "C" int sr_gfpgan_torgb_f32(const float* x, int64_t x_img_stride, const float* w, float wscale, const float* s,
                                   const float* bias, const float* skip, float* y, float* x_next, int64_t x_next_img_stride,
                                   const float* s_next, int n, int c, int h, int w_, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "sr_gfpgan_torgb_f32";
  SR_CHECK_ARG(x && w && s && bias && y && n > 0 && c > 0 && c % 8 == 0 && c <= 512 && h > 0 && w_ > 0, "%s: bad argument", who);
  SR_CHECK_ARG(!x_next == !s_next, "%s: x_next and s_next go together", who);
  SR_CHECK_ARG(!skip || (h % 2 == 0 && w_ % 2 == 0), "%s: a skip needs an even output size", who);
  SR_CHECK_ARG(((uintptr_t)x | (uintptr_t)x_next) % 16 == 0 && x_img_stride % 4 == 0 && x_next_img_stride % 4 == 0,
               "%s: x / x_next must be 16-byte aligned", who);
  SR_CHECK_ARG((long long)h * w_ * c < (1ll << 31) && n < 65536, "%s: image too large", who);
  RgbParams p = {};
  p.x = x;
  p.w = w;
  p.s = s;
  p.bias = bias;
  p.skip = skip;
  p.y = y;
  p.xn = x_next;
  p.sn = s_next;
  p.x_ns = x_img_stride;
  p.xn_ns = x_next_img_stride;
  p.C = c;
  p.H = h;
  p.W = w_;
  p.wscale = wscale;
  const long long HW = (long long)h * w_;
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 95, c, 3, n, h, w_, 6.0 * n * HW * c, 4.0 * n * HW * (c * (x_next ? 2 : 1) + 3 + (skip ? 1 : 0)));
  hipLaunchKernelGGL(gfp_torgb_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)n), dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("gfpgan torgb launch");
  return SR_OK;
}

extern "C" int sr_gfpgan_style_f32(const float* latent, int64_t latent_img_stride, int64_t latent_row_stride, int nsf,
                                   const sr_gfpgan_style_layer* layers, int n_layers, int n, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "sr_gfpgan_style_f32";
  SR_CHECK_ARG(latent && layers && nsf > 0 && nsf <= 1024 && n > 0 && n < 65536, "%s: bad argument", who);
  SR_CHECK_ARG(n_layers > 0 && n_layers <= SR_GFPGAN_MAX_LAYERS, "%s: n_layers=%d must be in [1, %d]", who, n_layers,
               SR_GFPGAN_MAX_LAYERS);
  StyleParams p = {};
  p.lat = latent;
  p.lat_ns = latent_img_stride;
  p.lat_rs = latent_row_stride;
  p.nsf = nsf;
  p.lin_scale = 1.f / sqrtf((float)nsf);
  double flops = 0.0, bytes = 0.0;
  for (int i = 0; i < n_layers; ++i) {
    const sr_gfpgan_style_layer& l = layers[i];
    SR_CHECK_ARG(l.mod_w && l.mod_b && l.s && l.cin > 0 && l.cin <= 512 && l.latent_index >= 0, "%s: bad layer %d", who, i);
    SR_CHECK_ARG(!l.q == !l.d && (!l.q || l.cout > 0), "%s: layer %d: q and d go together", who, i);
    p.L[i] = StyleLayerK{l.mod_w, l.mod_b, l.q, l.s, l.d, l.cin, l.cout, l.latent_index, l.wscale};
    flops += 2.0 * n * l.cin * (nsf + (l.q ? l.cout : 0));
    bytes += 4.0 * ((double)l.cin * nsf + (l.q ? (double)l.cout * l.cin : 0.0));
  }
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 91, nsf, n_layers, n, 1, 1, flops, bytes);
  hipLaunchKernelGGL(gfp_style_kernel, dim3((unsigned)n_layers, (unsigned)n), dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("gfpgan style launch");
  return SR_OK;
}

extern "C" int sr_gfpgan_norm_style_f32(const float* x, float* y, int n, int nsf, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && y && n > 0 && n < 65536 && nsf > 0 && nsf <= 1024, "sr_gfpgan_norm_style_f32: bad argument");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 96, nsf, nsf, n, 1, 1, 3.0 * n * nsf, 8.0 * n * nsf);
  hipLaunchKernelGGL(gfp_norm_kernel, dim3((unsigned)n), dim3(256), 0, stream, x, y, nsf);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("gfpgan norm_style launch");
  return SR_OK;
}
