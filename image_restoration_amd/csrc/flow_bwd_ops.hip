// The backward of SpyNet's building blocks on gfx950 (include/sr_hip_flow_bwd.h).
//
// Data gradient: the forward's implicit-GEMM body (flow_device.h, conv_body) with the mask epilogue compiled in, on a weight image
// that holds W flipped and transposed — a 7x7 convolution of dy.
//
// Weight gradient: D[cout][cin] += dy[cout][pixel] * x[pixel][cin] on v_mfma_f32_32x32x2_f32, the pixel pair as K.  All 49 taps of
// a 32 x 32 channel tile would be 784 accumulator registers, so a workgroup owns ONE TAP ROW (7 taps, 112 registers per wave) of
// the tile on a strip of 32 columns x RW rows; blockIdx.y enumerates (cout tile, cin tile, tap row), blockIdx.x the strips.  With
// the tap row fixed a dy row meets a single x row, so each wave stages just its own two rows, [pixel][32 channels] in LDS:
//   x row   38 pixels x 128 bytes = 4,864 bytes -> 5 LDS-DMA instructions (1 KiB each, the last lanes zero fill)
//   dy row  32 pixels x 128 bytes = 4,096 bytes -> 4
// double buffered: 2 x 4 waves x 9 KiB = 72 KiB, two workgroups per CU.  Lane (j, h) of the MFMA is channel j at pixel parity h: it
// reads dy[j] at the 16 pixels 2 m + h and x[j] at the 37 pixels h .. h + 36 into registers (conflict-free: 32 lanes x 4 bytes
// contiguous, the two halves 128 bytes apart) and tap tx of pixel pair m is x register 2 m + tx: 112 MFMAs from 53 LDS reads.
// Channel blocks the layer does not have and pixels outside the image are the zero fill of a buffer load beyond num_records.
#include <math.h>

#include "../../include/sr_hip_flow_bwd.h"
#include "flow_device.h"
#include "sr_internal.h"

using namespace flowdev;

namespace {

bool served(int cout, int cin) {
  return (cin == 8 && cout == 32) || (cin == 32 && cout == 64) || (cin == 64 && cout == 32) || (cin == 32 && cout == 16) ||
         (cin == 16 && cout == 2);
}
#define SR_PAIRS "(8, 32), (32, 64), (64, 32), (32, 16), (16, 2)"

// ------------------------------------------------------------------------------------------------------- data gradient
template <int COT, int PT>
__global__ __launch_bounds__(256, 2) void conv7x7_dgrad_f32_kernel(const C7MaskParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  conv_body<COT, PT, true>(p, smem);
}

// The image of conv_body for the transposed convolution: [dx group][dy block][tap row][tap column][COT][32 dx channels][8 dy
// channels] of W[dy channel][dx channel][6 - tap row][6 - tap column], then one zero per padded dx channel.
__global__ __launch_bounds__(256) void conv7x7_dgrad_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int cout, int cin,
                                                                 int COT, long long wfloats, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  if (idx >= wfloats) {
    out[idx] = 0.f;
    return;
  }
  const int dyb = (cout + 7) / 8;
  const int ch = (int)(idx & 7);
  const int i = (int)((idx >> 3) & 31);
  long long rest = idx >> 8;
  const int c = (int)(rest % COT);
  rest /= COT;
  const int tap = (int)(rest % 49);
  rest /= 49;
  const int cb = (int)(rest % dyb);
  const int g = (int)(rest / dyb);
  const int ci = (g * COT + c) * 32 + i;  // dx channel = the forward's input channel
  const int co = cb * 8 + ch;             // dy channel = the forward's output channel
  out[idx] = (co < cout && ci < cin) ? w[((long long)co * cin + ci) * 49 + (48 - tap)] : 0.f;
}

int dgrad_cot(int cin) { return cin == 64 ? 2 : 1; }
long long dgrad_weight_floats(int cout, int cin) {
  const int COT = dgrad_cot(cin);
  return (long long)sr::cdiv(cin, 32 * COT) * ((cout + 7) / 8) * 49 * COT * 256;
}
long long dgrad_zero_floats(int cin) { return (long long)sr::cdiv(cin, 32) * 32; }

// ----------------------------------------------------------------------------------------------------- weight gradient
constexpr int kWgX = 5 * 1024, kWgD = 4 * 1024, kWgWave = kWgX + kWgD, kWgLds = 2 * 4 * kWgWave;
constexpr int kTile = 7 * 1024;  // floats of one (channel tile, tap row) partial: [tap column][16 registers][64 lanes]

struct W7Params {
  const float* x;
  const float* dy;
  float* slab;   // [tile index][strip][7][1024]
  float* bslab;  // [cout tile][strip][64], null: no bias gradient
  long long x_ns, dy_ns;
  int xblocks, dyblocks, H, W, tiles_x, chunks, RW, IT, NP;
};

__global__ __launch_bounds__(256, 2) void conv7x7_wgrad_f32_kernel(const W7Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  int s = blockIdx.x;
  const int tx = s % p.tiles_x;
  s /= p.tiles_x;
  const int chunk = s % p.chunks, n = s / p.chunks;
  int T = blockIdx.y;
  const int ty = T % kKS;
  T /= kKS;
  const int it = T % p.IT, ct = T / p.IT;
  const int x0 = tx * 32, ybeg = chunk * p.RW, yend = min(ybeg + p.RW, p.H);
  const int HW = p.H * p.W;
  const bool do_bias = p.bslab != nullptr && ty == 3 && it == 0;  // tap row 3: the x row of a dy row is that row, never outside

  const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (long long)n * p.x_ns), 0,
                                                                        (unsigned)p.xblocks * (unsigned)HW * 32u, 0x00020000);
  const __amdgpu_buffer_rsrc_t d_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dy + (long long)n * p.dy_ns), 0,
                                                                        (unsigned)p.dyblocks * (unsigned)HW * 32u, 0x00020000);
  // Column part of this lane's offsets: slot q = unit * 64 + lane is (pixel q / 8, channel block (q / 2) % 4, 16-byte half q % 2),
  // so that the row lies in LDS as [pixel][32 channels].  0xffffffff: the slot is padding.
  unsigned xcol[5], dcol[4];
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int q = u * 64 + lane, pix = q >> 3, cb = it * 4 + ((q >> 1) & 3), gx = x0 - 3 + pix;
    xcol[u] = (pix < kXRow && gx >= 0 && gx < p.W && cb < p.xblocks) ? (unsigned)((cb * HW + gx) * 8 + (q & 1) * 4) * 4u : 0xffffffffu;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = u * 64 + lane, pix = q >> 3, cb = ct * 4 + ((q >> 1) & 3), gx = x0 + pix;
    dcol[u] = (gx < p.W && cb < p.dyblocks) ? (unsigned)((cb * HW + gx) * 8 + (q & 1) * 4) * 4u : 0xffffffffu;
  }

  auto rows = [&](int t, int& y, int& xr) {  // this wave's dy row and x row of step t; false: nothing to do
    y = ybeg + 4 * t + wave;
    xr = y + ty - 3;
    return y < yend && xr >= 0 && xr < p.H;
  };
  auto stage = [&](int buf, int t) {
    int y, xr;
    if (!rows(t, y, xr)) return;  // wave-uniform
    char* dst = smem + (buf * 4 + wave) * kWgWave;
    const unsigned xrow = (unsigned)(xr * p.W) * 32u, drow = (unsigned)(y * p.W) * 32u;
#pragma unroll
    for (int u = 0; u < 5; ++u) sr::blds16(x_rs, xcol[u] == 0xffffffffu ? 0xfffffff0u : xcol[u] + xrow, 0, dst + u * 1024);
#pragma unroll
    for (int u = 0; u < 4; ++u) sr::blds16(d_rs, dcol[u] == 0xffffffffu ? 0xfffffff0u : dcol[u] + drow, 0, dst + kWgX + u * 1024);
  };

  f32x16 acc[kKS];
#pragma unroll
  for (int a = 0; a < kKS; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
  float bsum = 0.f;

  const int rlane = h * 128 + j * 4;  // pixel parity h, channel j
  auto compute = [&](int buf, int t) {
    int y, xr;
    if (!rows(t, y, xr)) return;
    const char* xb = smem + (buf * 4 + wave) * kWgWave + rlane;
    const char* db = xb + kWgX;
    float xv[37], dv[16];
#pragma unroll
    for (int i = 0; i < 37; ++i) xv[i] = *(const float*)(xb + i * 128);
#pragma unroll
    for (int m = 0; m < 16; ++m) dv[m] = *(const float*)(db + m * 256);
#pragma unroll
    for (int m = 0; m < 16; ++m)
#pragma unroll
      for (int a = 0; a < kKS; ++a) acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[m], xv[2 * m + a], acc[a], 0, 0, 0);
    if (do_bias) {
#pragma unroll
      for (int m = 0; m < 16; ++m) bsum += dv[m];
    }
  };

  const int steps = p.RW / 4;
  stage(0, 0);
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    if (t + 1 < steps) stage((t + 1) & 1, t + 1);
    compute(t & 1, t);
    __syncthreads();  // drains the LDS-DMA issued above and frees the buffers just read
  }

  // ---- the four waves' tiles: (w0 + w2) + (w1 + w3), through LDS (every staging buffer is free after the last barrier)
  float* const ex = (float*)smem;               // 2 x [7][16][64] floats = 56 KiB
  float* const exb = (float*)(smem + 2 * kTile * 4);  // 2 x 64 floats
  if (wave >= 2) {
    float* o = ex + (wave - 2) * kTile + lane;
#pragma unroll
    for (int a = 0; a < kKS; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[(a * 16 + e) * 64] = acc[a][e];
    exb[(wave - 2) * 64 + lane] = bsum;
  }
  __syncthreads();
  if (wave < 2) {
    const float* o = ex + wave * kTile + lane;
#pragma unroll
    for (int a = 0; a < kKS; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][e] += o[(a * 16 + e) * 64];
    bsum += exb[wave * 64 + lane];
  }
  __syncthreads();
  if (wave == 1) {
    float* o = ex + lane;
#pragma unroll
    for (int a = 0; a < kKS; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[(a * 16 + e) * 64] = acc[a][e];
    exb[lane] = bsum;
  }
  __syncthreads();
  if (wave == 0) {
    const float* o = ex + lane;
    float* dst = p.slab + ((long long)blockIdx.y * p.NP + blockIdx.x) * kTile + lane;
#pragma unroll
    for (int a = 0; a < kKS; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) dst[(a * 16 + e) * 64] = acc[a][e] + o[(a * 16 + e) * 64];
    if (do_bias) p.bslab[((long long)ct * p.NP + blockIdx.x) * 64 + lane] = bsum + exb[lane];
  }
}

// One thread per element of the padded gradient (tile index, tap column, register, lane): the strips in ascending order, then
// scale, then store or add.  Register r of lane (j, h) is cout (r / 4) * 8 + h * 4 + r % 4, cin j of the tile.  The blocks behind
// the weight elements reduce the bias: strip s contributes (parity 0 + parity 1).
__global__ __launch_bounds__(256) void conv7x7_wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab,
                                                                   float* dw, float* db, int NP, int CT, int IT, int cout, int cin,
                                                                   float scale, int accumulate, int wblocks) {
  if ((int)blockIdx.x >= wblocks) {
    const int co = ((int)blockIdx.x - wblocks) * 256 + threadIdx.x;
    if (co >= cout) return;
    const float* s = bslab + ((long long)(co >> 5) * NP) * 64 + (co & 31);
    float sum = 0.f;
    for (int q = 0; q < NP; ++q) sum += s[(long long)q * 64] + s[(long long)q * 64 + 32];
    const float v = scale * sum;
    db[co] = accumulate ? db[co] + v : v;
    return;
  }
  const int idx = blockIdx.x * 256 + threadIdx.x;  // < CT * IT * 49 * 1024 <= 100,352
  const int e = idx & 1023, tx = (idx >> 10) % kKS, Tidx = idx / kTile;
  const int ty = Tidx % kKS, it = (Tidx / kKS) % IT, ct = Tidx / (kKS * IT);
  const float* s = slab + (long long)Tidx * NP * kTile + tx * 1024 + e;
  float sum = 0.f;
  for (int q = 0; q < NP; ++q) sum += s[(long long)q * kTile];
  const int lane = e & 63, r = e >> 6;
  const int ci = it * 32 + (lane & 31), co = ct * 32 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
  if (co >= cout || ci >= cin) return;
  const long long o = (((long long)co * cin + ci) * kKS + ty) * kKS + tx;
  const float v = scale * sum;
  dw[o] = accumulate ? dw[o] + v : v;
}

struct WgPlan {
  int CT, IT, TX, chunks, RW, NP;
  size_t wfloats, bfloats;
};
WgPlan wgrad_plan(int n, int h, int w, int cout, int cin) {
  WgPlan q;
  q.CT = sr::cdiv(cout, 32);
  q.IT = sr::cdiv(cin, 32);
  q.TX = sr::cdiv(w, 32);
  const long long per = (long long)n * q.TX * q.CT * q.IT * 7;
  long long chunks = (1024 + per - 1) / per;
  if (chunks < 1) chunks = 1;
  if (chunks > sr::cdiv(h, 4)) chunks = sr::cdiv(h, 4);
  q.RW = 4 * sr::cdiv(sr::cdiv(h, (int)chunks), 4);
  q.chunks = sr::cdiv(h, q.RW);
  q.NP = n * q.chunks * q.TX;
  q.wfloats = (size_t)q.NP * q.CT * q.IT * 49 * 1024;
  q.bfloats = (size_t)q.NP * q.CT * 64;
  return q;
}

// -------------------------------------------------------------------------------------------- level-input adjoint
// d_up = (g_res[0:2] + g_in[6:8]) + dflow: the dflow sum of flow_warp_bwd_dflow_kernel on (supp, up, g_in[3:6]) under border
__global__ __launch_bounds__(256) void spynet_level_dup_kernel(const float* __restrict__ supp, const float* __restrict__ up,
                                                               const float* __restrict__ g_in, const float* __restrict__ g_res,
                                                               float* __restrict__ d_up, int H, int W) {
  const int HW = H * W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int n = blockIdx.z;
  const int py = pix / W, px = pix - py * W;
  const long long b = ((long long)n * HW + pix) * 8;
  const float2 fl = *(const float2*)(up + b);
  const f32x4 ga = *(const f32x4*)(g_in + b), gb = *(const f32x4*)(g_in + b + 4);
  const float2 gr = *(const float2*)(g_res + b);
  int x0, y0;
  float fx, fy;
  bool gx_on, gy_on;
  warp_coord(fl.x, fl.y, px, py, H, W, 1, x0, y0, fx, fy, gx_on, gy_on);
  const Corners k = corners(x0, y0, H, W);
  const double ax = fx, ay = fy;
  const float gw[3] = {ga[3], gb[0], gb[1]};
  double sx = 0.0, sy = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* src = supp + ((long long)n * 3 + c) * HW;
    const double gv = gw[c];
    const double v00 = k.ok[0] ? src[k.off[0]] : 0.f, v01 = k.ok[1] ? src[k.off[1]] : 0.f;
    const double v10 = k.ok[2] ? src[k.off[2]] : 0.f, v11 = k.ok[3] ? src[k.off[3]] : 0.f;
    sx += gv * ((1.0 - ay) * (v01 - v00) + ay * (v11 - v10));
    sy += gv * ((1.0 - ax) * (v10 - v00) + ax * (v11 - v01));
  }
  if (!gx_on) sx = 0.0;
  if (!gy_on) sy = 0.0;
  *(float2*)(d_up + ((long long)n * HW + pix) * 2) = make_float2((gr.x + gb[2]) + (float)sx, (gr.y + gb[3]) + (float)sy);
}

// The fine indices that can have read coarse index ip: a superset, each candidate is then tested with the forward's own up_coord.
__device__ __forceinline__ void up_candidates(int ip, int dst_len, int src_len, int& lo, int& hi) {
  lo = 0;
  hi = dst_len - 1;
  if (src_len > 1) {
    const double r = (double)(dst_len - 1) / (double)(src_len - 1);
    lo = max(0, (int)floor((double)(ip - 1) * r) - 1);
    hi = min(dst_len - 1, (int)ceil((double)(ip + 1) * r) + 1);
  }
}
__device__ __forceinline__ double up_weight(int d, int ip, int dst_len, int src_len) {
  int i0, i1;
  double f;
  up_coord(d, dst_len, src_len, i0, i1, f);
  return (i0 == ip ? 1.0 - f : 0.0) + (i1 == ip ? f : 0.0);
}

__global__ __launch_bounds__(256) void spynet_level_upT_kernel(const float* __restrict__ d_up, float* __restrict__ g_prev, int H, int W) {
  const int Hp = H / 2, Wp = W / 2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Hp * Wp) return;
  const int n = blockIdx.z;
  const int yp = i / Wp, xp = i - yp * Wp;
  int ylo, yhi, xlo, xhi;
  up_candidates(yp, H, Hp, ylo, yhi);
  up_candidates(xp, W, Wp, xlo, xhi);
  double sx = 0.0, sy = 0.0;
  for (int y = ylo; y <= yhi; ++y) {
    const double wy = up_weight(y, yp, H, Hp);
    if (wy == 0.0) continue;
    for (int x = xlo; x <= xhi; ++x) {
      const double wx = up_weight(x, xp, W, Wp);
      if (wx == 0.0) continue;
      const float2 g = *(const float2*)(d_up + (((long long)n * H + y) * W + x) * 2);
      const double wgt = wy * wx;
      sx += wgt * (double)g.x;
      sy += wgt * (double)g.y;
    }
  }
  float* o = g_prev + ((long long)n * Hp * Wp + i) * 8;
  *(f32x4*)o = f32x4{(float)(2.0 * sx), (float)(2.0 * sy), 0.f, 0.f};
  *(f32x4*)(o + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ------------------------------------------------------------------------------------------------- resize adjoint
// source_coord of degrade_ops.hip (resize_bilinear_kernel), restated: every step a separate float32 operation
__device__ __forceinline__ void resize_coord(int d, int src_len, float scale, int& i0, int& i1, float& f) {
  const float s = (d + 0.5f) * scale - 0.5f;
  const float fl = floorf(s);
  i0 = (int)fl;
  f = s - fl;
  if (s < 0.f) {
    i0 = 0;
    f = 0.f;
  }
  if (i0 >= src_len - 1) {
    i0 = src_len - 1;
    f = 0.f;
  }
  i1 = min(i0 + 1, src_len - 1);
}
__device__ __forceinline__ double resize_weight(int d, int i, int src_len, float scale) {
  int i0, i1;
  float f;
  resize_coord(d, src_len, scale, i0, i1, f);
  return (i0 == i ? 1.0 - (double)f : 0.0) + (i1 == i ? (double)f : 0.0);
}
// destination indices that can have read source index i (a superset; the ends of the source take every clamped destination)
__device__ __forceinline__ void resize_candidates(int i, int src_len, int dst_len, int& lo, int& hi) {
  const double inv = (double)dst_len / (double)src_len;
  lo = i == 0 ? 0 : max(0, (int)floor(((double)i - 0.5) * inv - 0.5) - 2);
  hi = i >= src_len - 1 ? dst_len - 1 : min(dst_len - 1, (int)ceil(((double)i + 1.5) * inv - 0.5) + 2);
}

__global__ __launch_bounds__(256) void resize_bilinear_adjoint_kernel(const float* __restrict__ dy, float* __restrict__ dx, int Hs, int Ws,
                                                                      int Hd, int Wd) {
  const int xs = blockIdx.x * 64 + (threadIdx.x & 63), ys = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (xs >= Ws || ys >= Hs) return;
  const int plane = blockIdx.z;
  const float sy = (float)Hs / (float)Hd, sx = (float)Ws / (float)Wd;
  int ylo, yhi, xlo, xhi;
  resize_candidates(ys, Hs, Hd, ylo, yhi);
  resize_candidates(xs, Ws, Wd, xlo, xhi);
  const float* g = dy + (long long)plane * Hd * Wd;
  double sum = 0.0;
  for (int y = ylo; y <= yhi; ++y) {
    const double wy = resize_weight(y, ys, Hs, sy);
    if (wy == 0.0) continue;
    for (int x = xlo; x <= xhi; ++x) {
      const double wx = resize_weight(x, xs, Ws, sx);
      if (wx == 0.0) continue;
      sum += wy * wx * (double)g[(long long)y * Wd + x];
    }
  }
  dx[((long long)plane * Hs + ys) * Ws + xs] = (float)sum;
}

}  // namespace

extern "C" int sr_conv7x7_dgrad_instance(int cout, int cin) { return served(cout, cin) ? dgrad_cot(cin) - 1 : -1; }

extern "C" size_t sr_conv7x7_dgrad_packed_floats(int cout, int cin) {
  return served(cout, cin) ? (size_t)(dgrad_weight_floats(cout, cin) + dgrad_zero_floats(cin)) : 0;
}

extern "C" int sr_conv7x7_dgrad_pack_f32(const float* weight, int cout, int cin, float* packed, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(served(cout, cin), "sr_conv7x7_dgrad_pack_f32: (cin, cout) = (%d, %d) is not supported; supported: " SR_PAIRS, cin, cout);
  SR_CHECK_ARG(weight && packed, "sr_conv7x7_dgrad_pack_f32: null weight / packed");
  SR_CHECK_ARG(sr::aligned16(packed), "sr_conv7x7_dgrad_pack_f32: packed must be 16-byte aligned");
  const long long wf = dgrad_weight_floats(cout, cin), total = wf + dgrad_zero_floats(cin);
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 171, cin, cout, 1, 7, 7, 0.0, 4.0 * (total + 49.0 * cin * cout));
  hipLaunchKernelGGL(conv7x7_dgrad_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, weight, packed, cout, cin,
                     dgrad_cot(cin), wf, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_conv7x7_dgrad_pack_f32 launch");
  return SR_OK;
}

extern "C" int sr_conv7x7_dgrad_f32(const sr_conv7x7_dgrad_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_conv7x7_dgrad_f32: null descriptor");
  SR_CHECK_ARG(served(d->cout, d->cin), "sr_conv7x7_dgrad_f32: (cin, cout) = (%d, %d) is not supported; supported: " SR_PAIRS, d->cin,
               d->cout);
  SR_CHECK_ARG(d->dy && d->packed && d->dx, "sr_conv7x7_dgrad_f32: null dy / packed / dx");
  SR_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0, "sr_conv7x7_dgrad_f32: bad shape n=%d h=%d w=%d", d->n, d->h, d->w);
  SR_CHECK_ARG(sr::aligned16(d->dy) && sr::aligned16(d->packed) && sr::aligned16(d->dx) && sr::aligned16(d->mask),
               "sr_conv7x7_dgrad_f32: pointers must be 16-byte aligned");
  SR_CHECK_ARG(d->dy_img_stride % 4 == 0 && d->dx_img_stride % 4 == 0 && d->mask_img_stride % 4 == 0,
               "sr_conv7x7_dgrad_f32: image strides must be multiples of 4 floats");
  SR_CHECK_ARG(d->dx != d->dy, "sr_conv7x7_dgrad_f32: dx must not be dy");
  const long long hw = (long long)d->h * d->w;
  const int dyb = (d->cout + 7) / 8, dxb = d->cin / 8;
  SR_CHECK_ARG(hw * 32 * (dyb > dxb ? dyb : dxb) < (1ll << 31), "sr_conv7x7_dgrad_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(d->dy_img_stride >= hw * 8 * dyb && d->dx_img_stride >= hw * 8 * dxb && (!d->mask || d->mask_img_stride >= hw * 8 * dxb),
               "sr_conv7x7_dgrad_f32: an image stride is smaller than the image");
  const int inst = dgrad_cot(d->cin) - 1;
  C7MaskParams p = {};
  p.in = d->dy;
  p.w = d->packed;
  p.bias = d->packed + dgrad_weight_floats(d->cout, d->cin);
  p.out = d->dx;
  p.in_ns = d->dy_img_stride;
  p.out_ns = d->dx_img_stride;
  p.cin_blocks = dyb;
  p.cout_blocks = dxb;
  p.cout = d->cin;
  p.H = d->h;
  p.W = d->w;
  p.mask = d->mask;
  p.mask_ns = d->mask_img_stride;
  p.tiles_x = sr::cdiv(d->w, 32);
  p.tiles_y = sr::cdiv(d->h, inst == 1 ? 8 : 16);
  SR_CHECK_ARG((long long)p.tiles_x * p.tiles_y * d->n < (1ll << 31), "sr_conv7x7_dgrad_f32: grid too large");
  const void* kern = inst == 0 ? (const void*)conv7x7_dgrad_f32_kernel<1, 4> : (const void*)conv7x7_dgrad_f32_kernel<2, 2>;
  const int lds = inst == 0 ? conv_lds_bytes<1, 4>() : conv_lds_bytes<2, 2>();
  if (int rc = sr::ensure_dynamic_lds(kern, lds)) return rc;
  const dim3 grid((unsigned)(p.tiles_x * p.tiles_y * d->n), 1);
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * (double)hw;
    sr::prof_rec(stream, 169 + inst, d->cout, d->cin, d->n, d->h, d->w, 2.0 * 49.0 * d->cin * d->cout * px,
             4.0 * px * (dyb * 8.0 + d->cin * (d->mask ? 2 : 1)));
  }
  if (inst == 0)
    hipLaunchKernelGGL((conv7x7_dgrad_f32_kernel<1, 4>), grid, dim3(256), lds, stream, p);
  else
    hipLaunchKernelGGL((conv7x7_dgrad_f32_kernel<2, 2>), grid, dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_conv7x7_dgrad_f32 launch");
  return SR_OK;
}

extern "C" size_t sr_conv7x7_wgrad_slab_bytes(int n, int h, int w, int cout, int cin) {
  if (!served(cout, cin) || n <= 0 || h <= 0 || w <= 0) return 0;
  const WgPlan q = wgrad_plan(n, h, w, cout, cin);
  return 4 * (q.wfloats + q.bfloats);
}

extern "C" int sr_conv7x7_wgrad_f32(const sr_conv7x7_wgrad_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_conv7x7_wgrad_f32: null descriptor");
  SR_CHECK_ARG(served(d->cout, d->cin), "sr_conv7x7_wgrad_f32: (cin, cout) = (%d, %d) is not supported; supported: " SR_PAIRS, d->cin,
               d->cout);
  SR_CHECK_ARG(d->x && d->dy && d->dweight && d->slab, "sr_conv7x7_wgrad_f32: null x / dy / dweight / slab");
  SR_CHECK_ARG(d->n > 0 && d->n <= 65535 && d->h > 0 && d->w > 0, "sr_conv7x7_wgrad_f32: bad shape n=%d h=%d w=%d", d->n, d->h, d->w);
  SR_CHECK_ARG(sr::aligned16(d->x) && sr::aligned16(d->dy) && sr::aligned16(d->slab),
               "sr_conv7x7_wgrad_f32: x, dy and slab must be 16-byte aligned");
  SR_CHECK_ARG(((uintptr_t)d->dweight & 3u) == 0 && ((uintptr_t)d->dbias & 3u) == 0, "sr_conv7x7_wgrad_f32: dweight / dbias must be 4-byte aligned");
  SR_CHECK_ARG(d->x_img_stride % 4 == 0 && d->dy_img_stride % 4 == 0, "sr_conv7x7_wgrad_f32: image strides must be multiples of 4 floats");
  SR_CHECK_ARG(d->accumulate == 0 || d->accumulate == 1, "sr_conv7x7_wgrad_f32: accumulate must be 0 or 1");
  const long long hw = (long long)d->h * d->w;
  const int xb = d->cin / 8, dyb = (d->cout + 7) / 8;
  SR_CHECK_ARG(hw * 32 * (xb > dyb ? xb : dyb) < (1ll << 31), "sr_conv7x7_wgrad_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(d->x_img_stride >= hw * 8 * xb && d->dy_img_stride >= hw * 8 * dyb, "sr_conv7x7_wgrad_f32: an image stride is smaller than the image");
  const WgPlan q = wgrad_plan(d->n, d->h, d->w, d->cout, d->cin);
  const size_t need = 4 * (q.wfloats + q.bfloats);
  SR_CHECK_ARG(d->slab_bytes >= need, "sr_conv7x7_wgrad_f32: slab of %zu bytes, sr_conv7x7_wgrad_slab_bytes asks for %zu", d->slab_bytes, need);
  SR_CHECK_ARG((long long)q.NP < (1ll << 31) / 2, "sr_conv7x7_wgrad_f32: grid too large");
  W7Params p = {};
  p.x = d->x;
  p.dy = d->dy;
  p.slab = (float*)d->slab;
  p.bslab = d->dbias ? p.slab + q.wfloats : nullptr;
  p.x_ns = d->x_img_stride;
  p.dy_ns = d->dy_img_stride;
  p.xblocks = xb;
  p.dyblocks = dyb;
  p.H = d->h;
  p.W = d->w;
  p.tiles_x = q.TX;
  p.chunks = q.chunks;
  p.RW = q.RW;
  p.IT = q.IT;
  p.NP = q.NP;
  if (int rc = sr::ensure_dynamic_lds((const void*)conv7x7_wgrad_f32_kernel, kWgLds)) return rc;
  const bool prof = sr::prof_on();
  const double px = (double)d->n * (double)hw;
  if (prof) sr::prof_rec(stream, 172, d->cin, d->cout, d->n, d->h, d->w, 2.0 * 49.0 * d->cin * d->cout * px, 4.0 * px * (7.0 * d->cin + 7.0 * dyb * 8.0) + (double)need);
  hipLaunchKernelGGL(conv7x7_wgrad_f32_kernel, dim3((unsigned)q.NP, (unsigned)(q.CT * q.IT * 7)), dim3(256), kWgLds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_conv7x7_wgrad_f32 launch");
  const int wblocks = q.CT * q.IT * 49 * 4, bblocks = d->dbias ? sr::cdiv(d->cout, 256) : 0;
  if (prof) sr::prof_rec(stream, 173, d->cin, d->cout, d->n, d->h, d->w, (double)(q.wfloats + q.bfloats), (double)need + 8.0 * 49.0 * d->cin * d->cout);
  hipLaunchKernelGGL(conv7x7_wgrad_reduce_kernel, dim3((unsigned)(wblocks + bblocks)), dim3(256), 0, stream, (const float*)p.slab,
                     (const float*)p.bslab, d->dweight, d->dbias, q.NP, q.CT, q.IT, d->cout, d->cin, d->scale, d->accumulate, wblocks);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_conv7x7_wgrad_f32 reduction launch");
  return SR_OK;
}

extern "C" int sr_spynet_level_input_bwd_f32(const float* supp, const float* up, const float* g_in, const float* g_res, float* d_up,
                                             float* g_prev, int N, int H, int W, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(supp && up && g_in && g_res && d_up && g_prev, "sr_spynet_level_input_bwd_f32: null supp / up / g_in / g_res / d_up / g_prev");
  SR_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0, "sr_spynet_level_input_bwd_f32: bad shape N=%d H=%d W=%d", N, H, W);
  SR_CHECK_ARG(H % 2 == 0 && W % 2 == 0, "sr_spynet_level_input_bwd_f32: H=%d, W=%d must be even (the coarsest level has no incoming flow)", H, W);
  SR_CHECK_ARG((long long)H * W < (1ll << 28), "sr_spynet_level_input_bwd_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(sr::aligned16(up) && sr::aligned16(g_in) && sr::aligned16(g_res) && sr::aligned16(g_prev),
               "sr_spynet_level_input_bwd_f32: CB8 tensors must be 16-byte aligned");
  SR_CHECK_ARG(((uintptr_t)d_up & 7u) == 0, "sr_spynet_level_input_bwd_f32: d_up must be 8-byte aligned");
  SR_CHECK_ARG(g_prev != g_res && g_prev != g_in && g_prev != up, "sr_spynet_level_input_bwd_f32: g_prev must not be an input");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 174, 8, 2, N, H, W, 50.0 * N * H * W, 4.0 * N * H * W * (12.0 + 24.0 + 2.0));
  hipLaunchKernelGGL(spynet_level_dup_kernel, dim3((unsigned)sr::cdiv(H * W, 256), 1, (unsigned)N), dim3(256), 0, stream, supp, up, g_in,
                     g_res, d_up, H, W);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_spynet_level_input_bwd_f32 d_up launch");
  if (prof) sr::prof_rec(stream, 175, 2, 2, N, H / 2, W / 2, 4.0 * 9.0 * N * H * W, 4.0 * N * H * W * (2.0 + 2.0));
  hipLaunchKernelGGL(spynet_level_upT_kernel, dim3((unsigned)sr::cdiv((H / 2) * (W / 2), 256), 1, (unsigned)N), dim3(256), 0, stream,
                     (const float*)d_up, g_prev, H, W);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_spynet_level_input_bwd_f32 U^T launch");
  return SR_OK;
}

extern "C" int sr_resize_bilinear_adjoint_f32(const float* dy, float* dx, int planes, int Hs, int Ws, int Hd, int Wd, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(dy && dx, "sr_resize_bilinear_adjoint_f32: null dy / dx");
  SR_CHECK_ARG(planes > 0 && planes <= 65535 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0,
               "sr_resize_bilinear_adjoint_f32: bad shape [%d] %dx%d <- %dx%d (at most 65535 planes)", planes, Hs, Ws, Hd, Wd);
  SR_CHECK_ARG((long long)Hs * Ws < (1ll << 31) && (long long)Hd * Wd < (1ll << 31), "sr_resize_bilinear_adjoint_f32: image too large");
  SR_CHECK_ARG(dy != dx, "sr_resize_bilinear_adjoint_f32: dx must not be dy");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 176, 1, 1, planes, Hs, Ws, 3.0 * planes * Hd * Wd * 4.0, 4.0 * planes * ((double)Hs * Ws + (double)Hd * Wd));
  hipLaunchKernelGGL(resize_bilinear_adjoint_kernel, dim3((unsigned)sr::cdiv(Ws, 64), (unsigned)sr::cdiv(Hs, 4), (unsigned)planes), dim3(256),
                     0, stream, dy, dx, Hs, Ws, Hd, Wd);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_resize_bilinear_adjoint_f32 launch");
  return SR_OK;
}
