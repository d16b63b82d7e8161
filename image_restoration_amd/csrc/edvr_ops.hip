// EDVR (basicsr/archs/edvr_arch.py of the reference) on gfx950: the operators no other file of the library computes
// (include/sr_hip_edvr.h).
//
// Stride-2 3x3 convolution, pad 1: the implicit GEMM of ridnet_ops.hip's convd_f32_kernel (D[cout][pixel] += W[cout][k] *
// X[k][pixel] on v_mfma_f32_32x32x2_f32, CB8 layout, the same weight image, LDS-DMA staging through buffer descriptors,
// double-buffered chunks of one 8-channel block), copied rather than parameterised so that the stride-1 instruction streams stay
// as they are.  What differs is the staged source tile: an output tile of TH rows x 32 columns reads [2 TH + 1] source rows of
// 65 pixels, and tap (ty, tx) of output column j reads source column 2 j + tx of the tile.
//
// LDS layout and banks.  In the stride-1 layout ([row][pixel][8], 32 bytes per pixel) that access would put lane j at byte
// 64 j: the 16 lanes of a ds_read_b128 group would fall on 8 of the 16 16-byte slots of the 256-byte bank row, a 2-way
// conflict on every X read.  Instead each staged row holds its even source columns first (33 pixels, plane E) and its odd ones
// after them (32 pixels, plane O): [2 TH + 1][E 33 | O 32][8].  Taps tx = 0, 1, 2 of lane j then read pixel j of E, pixel j of O
// and pixel j + 1 of E: 32 lanes on 32 consecutive pixels of one plane, the access of the stride-1 kernels, with their swizzle
// (the two 16-byte halves of a pixel swapped where bit 3 of the pixel's index IN ITS PLANE is set).  For every tap the 16 lanes
// of each ds_read_b128 group ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and their upper-half twins) cover all 16 slots of the
// bank row once: no bank conflict; plane O's start (1056 bytes) and the row pitch (2080 bytes) only rotate a group's slots
// together.  The LDS-DMA writes the tile linearly, so the split costs nothing in LDS; in global memory a lane pair reads one
// 32-byte pixel and neighbouring pairs are 64 bytes apart, the E and O pieces of a row together covering whole lines.
//
// LDS bytes, all dynamic: 2 * (roundup1024((2 TH + 1) * 65 * 32) + 9 * COT * 1024), of the 160 KiB:
//   COT 1 / PT 1 57344,  COT 1 / PT 2 90112,  COT 2 / PT 1 75776,  COT 2 / PT 2 108544.
//
// The rest is memory-bound and pixel-local: zero insertion (the conv's backward), 3x3 / stride 2 max + average pooling and its
// gather-form adjoint, TSA's temporal correlation with its adjoint, TSA's gate with its adjoint.  One 16-byte half pixel or one
// pixel per thread; no atomics, fixed summation orders.
#include <algorithm>

#include "sr_internal.h"
#include "../../include/sr_hip_edvr.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

struct ConvS2Params {
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  long long in_ns, out_ns;
  int cin_blocks, cout_blocks;
  int H, W;    // source size
  int Ho, Wo;  // output size
  int tiles_x, tiles_y;
  float slope;
};

// One 32-column x (4*PT)-row x (32*COT)-cout output tile per workgroup of 4 waves.
template <int COT, int PT>
__global__ __launch_bounds__(256) void conv3x3s2_f32_kernel(const ConvS2Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = 4;
  constexpr int TH = NW * PT, XROWS = 2 * TH + 1, NE = 33, XROW = 65, XPIX = XROWS * XROW;
  constexpr int XBYTES = ((XPIX * 32 + 1023) / 1024) * 1024;
  constexpr int NXU = XBYTES / 1024, NWU = 9 * COT;
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
  const long long HWo = (long long)p.Ho * p.Wo;
  const float* in_n = p.in + (long long)n * p.in_ns;
  const float* wg = p.w + (size_t)cog * p.cin_blocks * W_CHUNK;

  // per-lane byte offsets of the X pieces this wave moves (beyond the buffer = zero padding), computed once per tile:
  // LDS pixel `pix` of the tile = (row, plane position); positions [0, 33) are the even source columns, [33, 65) the odd ones
  unsigned xvo[NXR];
#pragma unroll
  for (int r = 0; r < NXR; ++r) {
    const int u = r * NW + wave;
    const int q = u * 64 + lane;
    const int pix = q >> 1, half = q & 1;
    const int row = pix / XROW, pos = pix - row * XROW;
    const int idx = pos < NE ? pos : pos - NE;            // index in the plane
    const int col = pos < NE ? 2 * idx : 2 * idx + 1;     // source column of the tile
    const int gy = 2 * y0 - 1 + row, gx = 2 * x0 - 1 + col;
    const bool valid = pix < XPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
    const int hsw = half ^ ((idx >> 3) & 1);
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
      if (u < NXU) sr::blds16(x_rs, xvo[r], xso, xs + u * 1024);
    }
#pragma unroll
    for (int r = 0; r < NWR; ++r) {
      const int u = r * NW + wave;  // unit = tap * COT + cout sub-tile
      if (u < NWU) sr::blds16(w_rs, wvo, wso + (unsigned)(u * 256) * 4u, ws + u * 1024);
    }
  };

  f32x16 acc[COT][PT];
#pragma unroll
  for (int a = 0; a < COT; ++a)
#pragma unroll
    for (int b = 0; b < PT; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  // tap dx of lane j: plane E pixel j, plane O pixel j, plane E pixel j + 1
  const int xrow0 = wave * PT * 2 * XROW * 32;
  int xlane[3];
  xlane[0] = xrow0 + j * 32 + ((h ^ ((j >> 3) & 1)) * 16);
  xlane[1] = xrow0 + (NE + j) * 32 + ((h ^ ((j >> 3) & 1)) * 16);
  xlane[2] = xrow0 + (j + 1) * 32 + ((h ^ (((j + 1) >> 3) & 1)) * 16);
  const int wlane = j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  auto compute = [&](int buf) {
    const char* xb = smem + buf * STAGE;
    const char* ws = smem + buf * STAGE + XBYTES + wlane;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int tap = dy * 3 + dx;
        f32x4 a[COT], b[PT];
#pragma unroll
        for (int c = 0; c < COT; ++c) a[c] = *(const f32x4*)(ws + (tap * COT + c) * 1024);
#pragma unroll
        for (int r = 0; r < PT; ++r) b[r] = *(const f32x4*)(xb + xlane[dx] + (2 * r + dy) * XROW * 32);
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

  // epilogue: bias, LeakyReLU
  const int x = x0 + j;
  if (x >= p.Wo) return;
#pragma unroll
  for (int r = 0; r < PT; ++r) {
    const int y = y0 + wave * PT + r;
    if (y >= p.Ho) continue;
    const long long pixoff = (long long)y * p.Wo + x;
#pragma unroll
    for (int c = 0; c < COT; ++c) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = (cog * COT + c) * 4 + g;
        if (cb >= p.cout_blocks) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[c][r][g * 4 + e];
        if (p.bias) v += *(const f32x4*)(p.bias + cb * 8 + h * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
        *(f32x4*)(p.out + (long long)n * p.out_ns + (cb * HWo + pixoff) * 8 + h * 4) = v;
      }
    }
  }
}

template <int COT, int PT>
constexpr int conv3x3s2_lds_bytes() {
  return 2 * (((((2 * 4 * PT + 1) * 65 * 32) + 1023) / 1024) * 1024 + 9 * COT * 1024);
}

template <int COT, int PT>
int conv3x3s2_launch(const ConvS2Params& p, int n, int groups, const sr_conv3x3s2_desc* d, hipStream_t stream) {
  constexpr int lds = conv3x3s2_lds_bytes<COT, PT>();
  auto kern = conv3x3s2_f32_kernel<COT, PT>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, lds)) return rc;
  const bool prof = sr::prof_on();
  if (prof) {
    const double po = (double)n * p.Ho * p.Wo, pi = (double)n * p.H * p.W;
    sr::prof_rec(stream, 114, d->cin_pad, d->cout, n, p.H, p.W, 2.0 * 9 * d->cin_pad * d->cout * po, 4.0 * (pi * d->cin_pad + po * d->cout));
  }
  hipLaunchKernelGGL(kern, dim3(p.tiles_x * p.tiles_y * n, groups), dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("conv3x3s2_f32 launch");
  return SR_OK;
}

// The instance of one launch: COT = couts per weight-image group / 32; 8-row tiles (PT 2), 4-row tiles (PT 1) when the launch
// would not cover the chip once (the rule of sr_convd_f32, on the output size).  Shared by the launch and sr_conv3x3s2_lds_bytes.
struct S2Plan {
  int cot, pt, groups;
};

S2Plan s2_plan(int cout, int n, int in_h, int in_w) {
  const int ho = (in_h + 1) / 2, wo = (in_w + 1) / 2;
  const int gc = sr::group_couts(cout);
  S2Plan q;
  q.cot = gc / 32;
  q.groups = ((cout + 31) / 32 * 32) / gc;
  const bool small = (long long)sr::cdiv(wo, 32) * sr::cdiv(ho, 8) * n * q.groups < 256 && ho > 4;
  q.pt = small ? 1 : 2;
  return q;
}

// ------------------------------------------------------------------------------------------------ memory-bound kernels
// One 16-byte half pixel of a CB8 window [n][cb][h][w][8] per thread: i = ((n * cb + blk) * h * w + pix) * 2 + half.
struct HalfPix {
  long long n, pix;
  int blk, half;
};

__device__ __forceinline__ HalfPix half_pix(long long i, int cb, long long hw) {
  HalfPix q;
  q.half = (int)(i & 1);
  long long r = i >> 1;
  q.pix = r % hw;
  r /= hw;
  q.blk = (int)(r % cb);
  q.n = r / cb;
  return q;
}

__global__ __launch_bounds__(256) void cb8_zero_insert2_kernel(const float* __restrict__ dy, long long dy_ns, float* __restrict__ out,
                                                               long long out_ns, int cb, int h, int w, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const HalfPix q = half_pix(i, cb, (long long)h * w);
  const int y = (int)(q.pix / w), x = (int)(q.pix - (long long)y * w);
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!((y | x) & 1)) v = *(const f32x4*)(dy + q.n * dy_ns + (((long long)q.blk * ho + (y >> 1)) * wo + (x >> 1)) * 8 + q.half * 4);
  *(f32x4*)(out + q.n * out_ns + ((long long)q.blk * h * w + q.pix) * 8 + q.half * 4) = v;
}

// one output half pixel per thread; taps in row-major order, pad skipped (max) / counted as 0 (sum)
__global__ __launch_bounds__(256) void pool3x3s2_fwd_kernel(const float* __restrict__ x, long long x_ns, float* __restrict__ omax,
                                                            long long max_ns, float* __restrict__ oavg, long long avg_ns, int cb,
                                                            int h, int w, int ho, int wo, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const HalfPix q = half_pix(i, cb, (long long)ho * wo);
  const int oy = (int)(q.pix / wo), ox = (int)(q.pix - (long long)oy * wo);
  const float* xp = x + q.n * x_ns + (long long)q.blk * h * w * 8 + q.half * 4;
  const float ninf = -__builtin_inff();
  f32x4 m = {ninf, ninf, ninf, ninf}, s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ty = 0; ty < 3; ++ty) {
    const int yy = 2 * oy - 1 + ty;
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
      const int xx = 2 * ox - 1 + tx;
      if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
      const f32x4 v = *(const f32x4*)(xp + ((long long)yy * w + xx) * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
      s += v;
    }
  }
  const long long o = ((long long)q.blk * ho * wo + q.pix) * 8 + q.half * 4;
  *(f32x4*)(omax + q.n * max_ns + o) = m;
  *(f32x4*)(oavg + q.n * avg_ns + o) = s / 9.f;
}

// one source half pixel per thread
__global__ __launch_bounds__(256) void pool3x3s2_bwd_kernel(const float* __restrict__ x, long long x_ns, const float* __restrict__ gmax,
                                                            long long gmax_ns, const float* __restrict__ gavg, long long gavg_ns,
                                                            float* __restrict__ dx, long long dx_ns, int cb, int h, int w, int ho,
                                                            int wo, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const HalfPix q = half_pix(i, cb, (long long)h * w);
  const int y = (int)(q.pix / w), x0 = (int)(q.pix - (long long)y * w);
  const float* xp = x + q.n * x_ns + (long long)q.blk * h * w * 8 + q.half * 4;
  const float ninf = -__builtin_inff();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // windows oy with 2 oy - 1 <= y <= 2 oy + 1: y / 2 for an even y, (y - 1) / 2 and (y + 1) / 2 for an odd one
  const int oy0 = y >> 1, oy1 = (y + 1) >> 1, ox0 = x0 >> 1, ox1 = (x0 + 1) >> 1;
  for (int oy = oy0; oy <= oy1; ++oy) {
    if (oy >= ho) continue;
    for (int ox = ox0; ox <= ox1; ++ox) {
      if (ox >= wo) continue;
      f32x4 m = {ninf, ninf, ninf, ninf};
      int am[4] = {-1, -1, -1, -1};
#pragma unroll
      for (int ty = 0; ty < 3; ++ty) {
        const int yy = 2 * oy - 1 + ty;
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
          const int xx = 2 * ox - 1 + tx;
          if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
          const f32x4 v = *(const f32x4*)(xp + ((long long)yy * w + xx) * 8);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (v[e] > m[e]) {
              m[e] = v[e];
              am[e] = ty * 3 + tx;
            }
        }
      }
      const int mine = (y - (2 * oy - 1)) * 3 + (x0 - (2 * ox - 1));
      const long long o = ((long long)q.blk * ho * wo + (long long)oy * wo + ox) * 8 + q.half * 4;
      const f32x4 gm = *(const f32x4*)(gmax + q.n * gmax_ns + o);
      const f32x4 ga = *(const f32x4*)(gavg + q.n * gavg_ns + o);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (am[e] == mine) acc[e] += gm[e];
      acc += ga / 9.f;
    }
  }
  *(f32x4*)(dx + q.n * dx_ns + ((long long)q.blk * h * w + q.pix) * 8 + q.half * 4) = acc;
}

__device__ __forceinline__ float sigmoidf_(float s) { return 1.f / (1.f + expf(-s)); }

// one (frame, pixel) per thread
__global__ __launch_bounds__(256) void tsa_corr_fwd_kernel(const float* __restrict__ emb, long long emb_ns, const float* __restrict__ ref,
                                                           long long ref_ns, const float* __restrict__ al, long long al_ns,
                                                           float* __restrict__ prob, float* __restrict__ out, long long out_ns, int t,
                                                           int cb, long long hw, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long pix = i % hw, bt = i / hw, b = bt / t;
  const float* ep = emb + bt * emb_ns + pix * 8;
  const float* rp = ref + b * ref_ns + pix * 8;
  float s = 0.f;
  for (int k = 0; k < cb; ++k) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const f32x4 a = *(const f32x4*)(ep + k * hw * 8 + half * 4), r = *(const f32x4*)(rp + k * hw * 8 + half * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += a[e] * r[e];
    }
  }
  const float pr = sigmoidf_(s);
  prob[i] = pr;
  const float* ap = al + bt * al_ns + pix * 8;
  float* op = out + bt * out_ns + pix * 8;
  for (int k = 0; k < cb; ++k) {
#pragma unroll
    for (int half = 0; half < 2; ++half) *(f32x4*)(op + k * hw * 8 + half * 4) = *(const f32x4*)(ap + k * hw * 8 + half * 4) * pr;
  }
}

// one (frame, pixel) per thread: d_aligned, the correlation's gradient, d_emb
__global__ __launch_bounds__(256) void tsa_corr_bwd_kernel(const float* __restrict__ g, long long g_ns, const float* __restrict__ ref,
                                                           long long ref_ns, const float* __restrict__ al, long long al_ns,
                                                           const float* __restrict__ prob, float* __restrict__ dcorr,
                                                           float* __restrict__ dal, long long dal_ns, float* __restrict__ demb,
                                                           long long demb_ns, int t, int cb, long long hw, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long pix = i % hw, bt = i / hw, b = bt / t;
  const float pr = prob[i];
  const float* gp = g + bt * g_ns + pix * 8;
  const float* ap = al + bt * al_ns + pix * 8;
  float* dap = dal + bt * dal_ns + pix * 8;
  float s = 0.f;
  for (int k = 0; k < cb; ++k) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const f32x4 gv = *(const f32x4*)(gp + k * hw * 8 + half * 4), a = *(const f32x4*)(ap + k * hw * 8 + half * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += gv[e] * a[e];
      *(f32x4*)(dap + k * hw * 8 + half * 4) = gv * pr;
    }
  }
  const float ds = s * (pr * (1.f - pr));
  dcorr[i] = ds;
  const float* rp = ref + b * ref_ns + pix * 8;
  float* dep = demb + bt * demb_ns + pix * 8;
  for (int k = 0; k < cb; ++k) {
#pragma unroll
    for (int half = 0; half < 2; ++half) *(f32x4*)(dep + k * hw * 8 + half * 4) = *(const f32x4*)(rp + k * hw * 8 + half * 4) * ds;
  }
}

// one half pixel of d_emb_ref per thread: sum over the frames in ascending order
__global__ __launch_bounds__(256) void tsa_corr_bwd_ref_kernel(const float* __restrict__ emb, long long emb_ns,
                                                               const float* __restrict__ dcorr, float* __restrict__ dref,
                                                               long long dref_ns, int t, int cb, long long hw, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const HalfPix q = half_pix(i, cb, hw);
  const long long o = ((long long)q.blk * hw + q.pix) * 8 + q.half * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int f = 0; f < t; ++f) {
    const long long bt = q.n * t + f;
    acc += *(const f32x4*)(emb + bt * emb_ns + o) * dcorr[bt * hw + q.pix];
  }
  *(f32x4*)(dref + q.n * dref_ns + o) = acc;
}

__global__ __launch_bounds__(256) void tsa_gate_fwd_kernel(const float* __restrict__ feat, long long feat_ns, const float* __restrict__ attn,
                                                           long long attn_ns, const float* __restrict__ add, long long add_ns,
                                                           float* __restrict__ out, long long out_ns, long long per_img,
                                                           long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long n = i / per_img, o = (i - n * per_img) * 4;
  const f32x4 f = *(const f32x4*)(feat + n * feat_ns + o), a = *(const f32x4*)(attn + n * attn_ns + o);
  const f32x4 ad = *(const f32x4*)(add + n * add_ns + o);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (f[e] * sigmoidf_(a[e])) * 2.f + ad[e];
  *(f32x4*)(out + n * out_ns + o) = v;
}

__global__ __launch_bounds__(256) void tsa_gate_bwd_kernel(const float* __restrict__ g, long long g_ns, const float* __restrict__ feat,
                                                           long long feat_ns, const float* __restrict__ attn, long long attn_ns,
                                                           float* __restrict__ dfeat, long long df_ns, float* __restrict__ dattn,
                                                           long long da_ns, long long per_img, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long n = i / per_img, o = (i - n * per_img) * 4;
  const f32x4 gv = *(const f32x4*)(g + n * g_ns + o), f = *(const f32x4*)(feat + n * feat_ns + o);
  const f32x4 a = *(const f32x4*)(attn + n * attn_ns + o);
  f32x4 df, da;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float m = sigmoidf_(a[e]);
    df[e] = gv[e] * (2.f * m);
    da[e] = ((gv[e] * f[e]) * 2.f) * (m * (1.f - m));
  }
  *(f32x4*)(dfeat + n * df_ns + o) = df;
  *(f32x4*)(dattn + n * da_ns + o) = da;
}

bool aligned16(std::initializer_list<const void*> ptrs, std::initializer_list<long long> strides) {
  for (const void* q : ptrs)
    if ((uintptr_t)q % 16) return false;
  for (long long s : strides)
    if (s % 4) return false;
  return true;
}

bool grid_ok(long long total) { return total > 0 && (total + 255) / 256 < (1ll << 31); }

}  // namespace

#define EDVR_GRID(total) dim3((unsigned)(((total) + 255) / 256)), dim3(256), 0, stream

extern "C" int sr_conv3x3s2_f32(const sr_conv3x3s2_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_conv3x3s2_f32: null descriptor");
  SR_CHECK_ARG(d->in && d->wpacked && d->out, "sr_conv3x3s2_f32: null in/wpacked/out");
  SR_CHECK_ARG(d->cin_pad > 0 && d->cin_pad % 8 == 0, "sr_conv3x3s2_f32: cin_pad=%d must be a positive multiple of 8", d->cin_pad);
  SR_CHECK_ARG(d->cout > 0 && d->n > 0 && d->in_h > 0 && d->in_w > 0, "sr_conv3x3s2_f32: bad shape");
  SR_CHECK_ARG(aligned16({d->in, d->wpacked, d->bpacked, d->out}, {d->in_img_stride, d->out_img_stride}),
               "sr_conv3x3s2_f32: pointers must be 16-byte aligned");
  const int cin_blocks = d->cin_pad / 8, cout_blocks = (d->cout + 7) / 8;
  const long long blocks = std::max(cin_blocks, cout_blocks);
  SR_CHECK_ARG((long long)d->in_h * d->in_w * 8 * blocks * 4 < (1ll << 32), "sr_conv3x3s2_f32: image too large for 32-bit offsets");
  ConvS2Params p = {};
  p.in = d->in;
  p.w = d->wpacked;
  p.bias = d->bpacked;
  p.out = d->out;
  p.in_ns = d->in_img_stride;
  p.out_ns = d->out_img_stride;
  p.cin_blocks = cin_blocks;
  p.cout_blocks = cout_blocks;
  p.H = d->in_h;
  p.W = d->in_w;
  p.Ho = (d->in_h + 1) / 2;
  p.Wo = (d->in_w + 1) / 2;
  p.tiles_x = sr::cdiv(p.Wo, 32);
  p.slope = d->act_slope;
  const S2Plan plan = s2_plan(d->cout, d->n, d->in_h, d->in_w);
  SR_CHECK_ARG((long long)p.tiles_x * sr::cdiv(p.Ho, 4) * d->n < (1ll << 31), "sr_conv3x3s2_f32: grid too large");
  p.tiles_y = sr::cdiv(p.Ho, 4 * plan.pt);
  if (plan.cot == 2)
    return plan.pt == 1 ? conv3x3s2_launch<2, 1>(p, d->n, plan.groups, d, stream) : conv3x3s2_launch<2, 2>(p, d->n, plan.groups, d, stream);
  return plan.pt == 1 ? conv3x3s2_launch<1, 1>(p, d->n, plan.groups, d, stream) : conv3x3s2_launch<1, 2>(p, d->n, plan.groups, d, stream);
}

extern "C" size_t sr_conv3x3s2_lds_bytes(int cout, int n, int in_h, int in_w) {
  if (cout <= 0 || n <= 0 || in_h <= 0 || in_w <= 0) return 0;
  const S2Plan plan = s2_plan(cout, n, in_h, in_w);
  if (plan.cot == 2) return plan.pt == 1 ? conv3x3s2_lds_bytes<2, 1>() : conv3x3s2_lds_bytes<2, 2>();
  return plan.pt == 1 ? conv3x3s2_lds_bytes<1, 1>() : conv3x3s2_lds_bytes<1, 2>();
}

extern "C" int sr_cb8_zero_insert2_f32(const float* dy, int64_t dy_ns, float* out, int64_t out_ns, int n, int cb, int h, int w,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(dy && out && n > 0 && cb > 0 && h > 0 && w > 0, "sr_cb8_zero_insert2_f32: bad argument");
  SR_CHECK_ARG(aligned16({dy, out}, {dy_ns, out_ns}), "sr_cb8_zero_insert2_f32: pointers must be 16-byte aligned");
  const long long total = (long long)n * cb * h * w * 2;
  SR_CHECK_ARG(grid_ok(total), "sr_cb8_zero_insert2_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 115, cb * 8, cb * 8, n, h, w, 0.0, 4.0 * n * cb * 8 * ((double)h * w + (double)((h + 1) / 2) * ((w + 1) / 2)));
  hipLaunchKernelGGL(cb8_zero_insert2_kernel, EDVR_GRID(total), dy, (long long)dy_ns, out, (long long)out_ns, cb, h, w, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("cb8_zero_insert2 launch");
  return SR_OK;
}

extern "C" int sr_pool3x3s2_fwd_f32(const float* x, int64_t x_ns, float* out_max, int64_t max_ns, float* out_avg, int64_t avg_ns,
                                    int n, int cb, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && out_max && out_avg && n > 0 && cb > 0 && h > 0 && w > 0, "sr_pool3x3s2_fwd_f32: bad argument");
  SR_CHECK_ARG(aligned16({x, out_max, out_avg}, {x_ns, max_ns, avg_ns}), "sr_pool3x3s2_fwd_f32: pointers must be 16-byte aligned");
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const long long total = (long long)n * cb * ho * wo * 2;
  SR_CHECK_ARG(grid_ok(total), "sr_pool3x3s2_fwd_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 116, cb * 8, cb * 16, n, h, w, 17.0 * n * cb * 8 * ho * wo, 4.0 * n * cb * 8 * ((double)h * w + 2.0 * ho * wo));
  hipLaunchKernelGGL(pool3x3s2_fwd_kernel, EDVR_GRID(total), x, (long long)x_ns, out_max, (long long)max_ns, out_avg,
                     (long long)avg_ns, cb, h, w, ho, wo, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("pool3x3s2_fwd launch");
  return SR_OK;
}

extern "C" int sr_pool3x3s2_bwd_f32(const float* x, int64_t x_ns, const float* g_max, int64_t gmax_ns, const float* g_avg,
                                    int64_t gavg_ns, float* dx, int64_t dx_ns, int n, int cb, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && g_max && g_avg && dx && n > 0 && cb > 0 && h > 0 && w > 0, "sr_pool3x3s2_bwd_f32: bad argument");
  SR_CHECK_ARG(aligned16({x, g_max, g_avg, dx}, {x_ns, gmax_ns, gavg_ns, dx_ns}), "sr_pool3x3s2_bwd_f32: pointers must be 16-byte aligned");
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const long long total = (long long)n * cb * h * w * 2;
  SR_CHECK_ARG(grid_ok(total), "sr_pool3x3s2_bwd_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 117, cb * 16, cb * 8, n, h, w, 12.0 * n * cb * 8 * h * w, 4.0 * n * cb * 8 * (2.0 * h * w + 2.0 * ho * wo));
  hipLaunchKernelGGL(pool3x3s2_bwd_kernel, EDVR_GRID(total), x, (long long)x_ns, g_max, (long long)gmax_ns, g_avg, (long long)gavg_ns,
                     dx, (long long)dx_ns, cb, h, w, ho, wo, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("pool3x3s2_bwd launch");
  return SR_OK;
}

extern "C" int sr_tsa_corr_fwd_f32(const float* emb, int64_t emb_ns, const float* emb_ref, int64_t ref_ns, const float* aligned,
                                   int64_t al_ns, float* prob, float* out, int64_t out_ns, int b, int t, int c, int h, int w,
                                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(emb && emb_ref && aligned && prob && out, "sr_tsa_corr_fwd_f32: null pointer");
  SR_CHECK_ARG(b > 0 && t > 0 && c > 0 && c % 8 == 0 && h > 0 && w > 0, "sr_tsa_corr_fwd_f32: bad shape (c=%d must be a multiple of 8)", c);
  SR_CHECK_ARG(aligned16({emb, emb_ref, aligned, out}, {emb_ns, ref_ns, al_ns, out_ns}) && (uintptr_t)prob % 4 == 0,
               "sr_tsa_corr_fwd_f32: pointers must be 16-byte aligned");
  const long long hw = (long long)h * w, total = (long long)b * t * hw;
  SR_CHECK_ARG(grid_ok(total), "sr_tsa_corr_fwd_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 118, c, c, b * t, h, w, 3.0 * total * c, 4.0 * total * (3.0 * c + 1) + 4.0 * b * hw * c);
  hipLaunchKernelGGL(tsa_corr_fwd_kernel, EDVR_GRID(total), emb, (long long)emb_ns, emb_ref, (long long)ref_ns, aligned,
                     (long long)al_ns, prob, out, (long long)out_ns, t, c / 8, hw, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("tsa_corr_fwd launch");
  return SR_OK;
}

extern "C" int sr_tsa_corr_bwd_f32(const float* g, int64_t g_ns, const float* emb, int64_t emb_ns, const float* emb_ref,
                                   int64_t ref_ns, const float* aligned, int64_t al_ns, const float* prob, float* dcorr,
                                   float* d_aligned, int64_t da_ns, float* d_emb, int64_t de_ns, float* d_emb_ref, int64_t dr_ns, int b,
                                   int t, int c, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(g && emb && emb_ref && aligned && prob && dcorr && d_aligned && d_emb && d_emb_ref, "sr_tsa_corr_bwd_f32: null pointer");
  SR_CHECK_ARG(b > 0 && t > 0 && c > 0 && c % 8 == 0 && h > 0 && w > 0, "sr_tsa_corr_bwd_f32: bad shape (c=%d must be a multiple of 8)", c);
  SR_CHECK_ARG(aligned16({g, emb, emb_ref, aligned, d_aligned, d_emb, d_emb_ref}, {g_ns, emb_ns, ref_ns, al_ns, da_ns, de_ns, dr_ns}) &&
                   ((uintptr_t)prob | (uintptr_t)dcorr) % 4 == 0,
               "sr_tsa_corr_bwd_f32: pointers must be 16-byte aligned");
  const long long hw = (long long)h * w, total = (long long)b * t * hw, total_ref = (long long)b * (c / 8) * hw * 2;
  SR_CHECK_ARG(grid_ok(total) && grid_ok(total_ref), "sr_tsa_corr_bwd_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 119, c, c, b * t, h, w, 4.0 * total * c, 4.0 * total * (4.0 * c + 2) + 4.0 * b * hw * c);
  hipLaunchKernelGGL(tsa_corr_bwd_kernel, EDVR_GRID(total), g, (long long)g_ns, emb_ref, (long long)ref_ns, aligned, (long long)al_ns,
                     prob, dcorr, d_aligned, (long long)da_ns, d_emb, (long long)de_ns, t, c / 8, hw, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("tsa_corr_bwd launch");
  if (prof) sr::prof_rec(stream, 120, c, c, b, h, w, 2.0 * total * c, 4.0 * (total * (c + 1.0) + (double)b * hw * c));
  hipLaunchKernelGGL(tsa_corr_bwd_ref_kernel, EDVR_GRID(total_ref), emb, (long long)emb_ns, (const float*)dcorr, d_emb_ref,
                     (long long)dr_ns, t, c / 8, hw, total_ref);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("tsa_corr_bwd_ref launch");
  return SR_OK;
}

extern "C" int sr_tsa_gate_fwd_f32(const float* feat, int64_t feat_ns, const float* attn, int64_t attn_ns, const float* attn_add,
                                   int64_t add_ns, float* out, int64_t out_ns, int n, int cb, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(feat && attn && attn_add && out && n > 0 && cb > 0 && h > 0 && w > 0, "sr_tsa_gate_fwd_f32: bad argument");
  SR_CHECK_ARG(aligned16({feat, attn, attn_add, out}, {feat_ns, attn_ns, add_ns, out_ns}), "sr_tsa_gate_fwd_f32: pointers must be 16-byte aligned");
  const long long per_img = (long long)cb * h * w * 2, total = per_img * n;
  SR_CHECK_ARG(grid_ok(total), "sr_tsa_gate_fwd_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 121, cb * 8, cb * 8, n, h, w, 8.0 * total * 4, 4.0 * 4 * total * 4);
  hipLaunchKernelGGL(tsa_gate_fwd_kernel, EDVR_GRID(total), feat, (long long)feat_ns, attn, (long long)attn_ns, attn_add,
                     (long long)add_ns, out, (long long)out_ns, per_img, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("tsa_gate_fwd launch");
  return SR_OK;
}

extern "C" int sr_tsa_gate_bwd_f32(const float* g, int64_t g_ns, const float* feat, int64_t feat_ns, const float* attn, int64_t attn_ns,
                                   float* d_feat, int64_t df_ns, float* d_attn, int64_t da_ns, int n, int cb, int h, int w,
                                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(g && feat && attn && d_feat && d_attn && n > 0 && cb > 0 && h > 0 && w > 0, "sr_tsa_gate_bwd_f32: bad argument");
  SR_CHECK_ARG(aligned16({g, feat, attn, d_feat, d_attn}, {g_ns, feat_ns, attn_ns, df_ns, da_ns}),
               "sr_tsa_gate_bwd_f32: pointers must be 16-byte aligned");
  const long long per_img = (long long)cb * h * w * 2, total = per_img * n;
  SR_CHECK_ARG(grid_ok(total), "sr_tsa_gate_bwd_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 122, cb * 8, cb * 8, n, h, w, 10.0 * total * 4, 4.0 * 5 * total * 4);
  hipLaunchKernelGGL(tsa_gate_bwd_kernel, EDVR_GRID(total), g, (long long)g_ns, feat, (long long)feat_ns, attn, (long long)attn_ns,
                     d_feat, (long long)df_ns, d_attn, (long long)da_ns, per_img, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("tsa_gate_bwd launch");
  return SR_OK;
}
