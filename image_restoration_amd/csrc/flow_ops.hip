// Optical flow building blocks on gfx950 (include/sr_hip_flow.h): flow warping and the pieces of SpyNet.
//
// Reference: flow_warp (basicsr/archs/arch_util.py:112-143) builds a normalised grid and calls F.grid_sample; SpyNet
// (basicsr/archs/spynet_arch.py) runs, per pyramid level, F.interpolate + flow_warp + torch.cat and five nn.Conv2d(k7, s1, p3)
// with ReLUs.  Here a level is one launch for its input block and five launches of the 7x7 convolution below.
//
// 7x7 convolution: implicit GEMM  D[cout][pixel] += W[cout][k] * X[k][pixel],  k = (cin, tap), on v_mfma_f32_32x32x2_f32, in the
// manner of conv_f32_kernel (conv_f32.hip): A = weights, B = activations, the pixel on the lane and 4 consecutive couts in 4
// consecutive accumulator registers, so that a quad is one 16-byte store into CB8.  Workgroup = 4 waves, output tile =
// (4 * PT rows) x 32 columns x (32 * COT couts); wave w owns PT rows.  K = 49 * cin is walked in chunks of (one 8-channel block,
// one TAP ROW): the halo'd X tile [TH + 6][38][8] is staged once per channel block, the weights [7 taps][32 * COT][8] once per
// chunk, both by LDS-DMA through buffer descriptors (1 KiB per wave-instruction), both double buffered, one barrier per chunk.
// A whole [49][32 * COT][8] weight chunk would be 49 * COT KiB per buffer; by tap rows it is 7 * COT KiB, and
//   <1, 4>: 2 * (27 + 7) KiB = 68 KiB      <2, 2>: 2 * (17 + 14) KiB = 62 KiB      few-cout: 2 * (27 + 7) KiB = 68 KiB
// so two workgroups share a CU's 160 KiB (two waves per SIMD, 64 accumulator registers each).  The 3-pixel zero padding is the
// hardware's zero fill of a buffer load beyond num_records: pad lanes carry an offset outside the descriptor.
// Per chunk and wave: 7 * (COT + PT) ds_read_b128 feed 28 * COT * PT MFMAs of 64 cycles.
#include <math.h>

#include "../../include/sr_hip_flow.h"
#include "flow_device.h"
#include "sr_internal.h"

using namespace flowdev;  // the conv body, the warp rule and the level coordinate, shared with flow_bwd_ops.hip

namespace {

// ------------------------------------------------------------------------------------------------------------ conv 7x7
// The body described above is conv_body of flow_device.h (KS = 7 from C7Params), shared with the data gradient
// (flow_bwd_ops.hip) and TOFlow's 9x9 (tof_ops.hip); MASK = false here.
template <int COT, int PT>
__global__ __launch_bounds__(256, 2) void conv7x7_f32_kernel(const C7Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  conv_body<COT, PT, false>(p, smem);
}

// Few output channels (the last conv of a level: 16 -> 2) on v_mfma_f32_4x4x1_16b_f32, after conv_fewcout_f32_kernel: the 32x32
// tile would pad 2 couts to 32, the 16-block 4x4x1 form pads to 4.  Block b = lane / 4 computes D[4 couts][4 pixels] +=
// A[4 couts][1] * B[1][4 pixels], so lane l IS pixel l of a 64-pixel group and holds its 4 couts in 4 registers.  Tile 16 rows x
// 32 columns; wave w owns rows 4w .. 4w + 3 as two 64-pixel groups that share the weight fragments.  A chunk is one 8-channel
// block with all 49 taps: X as above, the weights [49][4 couts][8] = 6,272 bytes.
__global__ __launch_bounds__(256, 2) void conv7x7_fewcout_f32_kernel(const C7Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TH = 16, XPIX = (TH + kKS - 1) * kXRow, NT = kKS * kKS;
  constexpr int XBYTES = ((XPIX * 32 + 1023) / 1024) * 1024, NXU = XBYTES / 1024, NXR = (NXU + 3) / 4;
  constexpr int WREAL = NT * 4 * 32, WBYTES = ((WREAL + 1023) / 1024) * 1024, NWU = WBYTES / 1024, NWR = (NWU + 3) / 4;
  constexpr int STAGE = XBYTES + WBYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int t = xcd_tile(gridDim.x, blockIdx.x);
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y, n = t / p.tiles_y;
  const int x0 = tx * 32, y0 = ty * TH;
  const int HW = p.H * p.W;
  const float* in_n = p.in + (long long)n * p.in_ns;

  unsigned xvo[NXR], wvo[NWR];
  x_offsets<NXR, XPIX>(xvo, wave, lane, x0, y0, p.H, p.W);
#pragma unroll
  for (int r = 0; r < NWR; ++r) {
    const unsigned q = (unsigned)((r * 4 + wave) * 64 + lane) * 16u;
    wvo[r] = q < (unsigned)WREAL ? q : 0xfffffff0u;
  }
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)in_n, 0, (unsigned)p.cin_blocks * (unsigned)HW * 32u, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (unsigned)p.cin_blocks * (unsigned)WREAL, 0x00020000);
  auto stage = [&](int buf, int cb) {
    char* xs = smem + buf * STAGE;
    const unsigned xso = (unsigned)cb * (unsigned)HW * 32u, wso = (unsigned)cb * (unsigned)WREAL;
#pragma unroll
    for (int r = 0; r < NXR; ++r) {
      const int u = r * 4 + wave;
      if (u < NXU) sr::blds16(x_rs, xvo[r], xso, xs + u * 1024);
    }
#pragma unroll
    for (int r = 0; r < NWR; ++r) {
      const int u = r * 4 + wave;
      if (u < NWU) sr::blds16(w_rs, wvo[r], wso, xs + XBYTES + u * 1024);
    }
  };

  f32x4 acc[2];
  acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int prow = lane >> 5, pcol = lane & 31;
  const int xlane = ((wave * 4 + prow) * kXRow + pcol) * 32;  // this lane's pixel, group 0, tap (0, 0)
  const int wlane = (lane & 3) * 32;                          // this lane's cout row of the weight chunk

  auto compute = [&](int buf) {
    const char* xs = smem + buf * STAGE + xlane;
    const char* ws = smem + buf * STAGE + XBYTES + wlane;
#pragma unroll 1
    for (int dy = 0; dy < kKS; ++dy)
#pragma unroll
      for (int dx = 0; dx < kKS; ++dx) {
        const int tap = dy * kKS + dx;
        const f32x4 w0 = *(const f32x4*)(ws + tap * 128), w1 = *(const f32x4*)(ws + tap * 128 + 16);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const char* xp = xs + ((2 * g + dy) * kXRow + dx) * 32;
          const int sw = (((pcol + dx) >> 3) & 1) * 16;  // where this column's first half lives
          const f32x4 a0 = *(const f32x4*)(xp + sw), a1 = *(const f32x4*)(xp + (sw ^ 16));
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(w0[e], a0[e], acc[g], 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(w1[e], a1[e], acc[g], 0, 0, 0);
        }
      }
  };

  stage(0, 0);
  __syncthreads();
  for (int c = 0; c < p.cin_blocks; ++c) {
    if (c + 1 < p.cin_blocks) stage((c + 1) & 1, c + 1);
    compute(c & 1);
    __syncthreads();
  }
  // epilogue: bias, ReLU, res1; one CB8 block, channels >= cout written 0
  const int x = x0 + pcol;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int y = y0 + wave * 4 + 2 * g + prow;
    if (y >= p.H || x >= p.W) continue;
    const long long off = ((long long)y * p.W + x) * 8;
    f32x4 v = acc[g] + *(const f32x4*)p.bias;
    if (p.relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
    }
    if (p.res1) v += *(const f32x4*)(p.res1 + (long long)n * p.res1_ns + off);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e >= p.cout) v[e] = 0.f;
    float* o = p.out + (long long)n * p.out_ns + off;
    *(f32x4*)o = v;
    *(f32x4*)(o + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// Weight images.  Instances 0 / 1: [cout group][cin block][tap row][tap column][COT][32 couts][8 channels]; instance 2:
// [cin block][49 taps][4 couts][8 channels]; then the bias, padded with zeros.
__global__ __launch_bounds__(256) void conv7x7_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out, int cout, int cin, int inst, long long wfloats,
                                                           long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  if (idx >= wfloats) {
    const int b = (int)(idx - wfloats);
    out[idx] = (bias && b < cout) ? bias[b] : 0.f;
    return;
  }
  const int cinb = (cin + 7) / 8;
  const int ch = (int)(idx & 7);
  int co, cb, tap;
  if (inst == 2) {
    co = (int)((idx >> 3) & 3);
    const long long rest = idx >> 5;
    tap = (int)(rest % 49);
    cb = (int)(rest / 49);
  } else {
    const int COT = inst + 1;
    const int i = (int)((idx >> 3) & 31);
    long long rest = idx >> 8;
    const int c = (int)(rest % COT);
    rest /= COT;
    tap = (int)(rest % 49);  // tap row * 7 + tap column
    rest /= 49;
    cb = (int)(rest % cinb);
    const int cog = (int)(rest / cinb);
    co = (cog * COT + c) * 32 + i;
  }
  const int ci = cb * 8 + ch;
  out[idx] = (co < cout && ci < cin) ? w[((long long)co * cin + ci) * 49 + tap] : 0.f;
}

long long conv7x7_weight_floats(int cout, int cin, int inst) {
  const long long cinb = (cin + 7) / 8;
  if (inst == 2) return cinb * 49 * 32;
  const int COT = inst + 1;
  return (long long)sr::cdiv(cout, 32 * COT) * cinb * 49 * COT * 256;
}
long long conv7x7_bias_floats(int cout, int inst) { return inst == 2 ? 32 : (long long)sr::cdiv(cout, 32 * (inst + 1)) * (inst + 1) * 32; }

constexpr int kFewLds = 2 * (((((16 + kKS - 1) * kXRow * 32 + 1023) / 1024) * 1024) + ((49 * 128 + 1023) / 1024) * 1024);

// -------------------------------------------------------------------------------------------------------- flow warping
// grid (ceil(HW / 256), ceil(C / 8), N): a thread warps up to 8 channels of one pixel
template <bool CB8>
__global__ __launch_bounds__(256) void flow_warp_kernel(const float* __restrict__ x, const float* __restrict__ flow,
                                                        float* __restrict__ out, int C, int H, int W, int border) {
  const int HW = H * W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int cg = blockIdx.y, n = blockIdx.z, CG = gridDim.y;
  const int py = pix / W, px = pix - py * W;
  const float2 fl = *(const float2*)(flow + ((long long)n * HW + pix) * 2);
  int x0, y0;
  float fx, fy;
  bool gx_on, gy_on;
  const bool any = warp_coord(fl.x, fl.y, px, py, H, W, border, x0, y0, fx, fy, gx_on, gy_on);
  Corners k = {};
  if (any) k = corners(x0, y0, H, W);
  const int nc = min(8, C - cg * 8);
  if (CB8) {
    const float* src = x + ((long long)n * CG + cg) * HW * 8;
    float v[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
      if (any && k.ok[q]) {
        a = *(const f32x4*)(src + (long long)k.off[q] * 8);
        b = *(const f32x4*)(src + (long long)k.off[q] * 8 + 4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[q][e] = a[e];
        v[q][4 + e] = b[e];
      }
    }
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (any && e < nc) ? blend(v[0][e], v[1][e], v[2][e], v[3][e], fx, fy) : 0.f;
    float* dst = out + (((long long)n * CG + cg) * HW + pix) * 8;
    *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
    *(f32x4*)(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
  } else {
    for (int e = 0; e < nc; ++e) {
      const long long plane = ((long long)n * C + cg * 8 + e) * HW;
      float r = 0.f;
      if (any) {
        const float* src = x + plane;
        r = blend(k.ok[0] ? src[k.off[0]] : 0.f, k.ok[1] ? src[k.off[1]] : 0.f, k.ok[2] ? src[k.off[2]] : 0.f,
                  k.ok[3] ? src[k.off[3]] : 0.f, fx, fy);
      }
      out[plane + pix] = r;
    }
  }
}

// dx scatter: same decomposition as the forward
template <bool CB8>
__global__ __launch_bounds__(256) void flow_warp_bwd_dx_kernel(const float* __restrict__ flow, const float* __restrict__ g,
                                                               float* dx, int C, int H, int W, int border) {
  const int HW = H * W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int cg = blockIdx.y, n = blockIdx.z, CG = gridDim.y;
  const int py = pix / W, px = pix - py * W;
  const float2 fl = *(const float2*)(flow + ((long long)n * HW + pix) * 2);
  int x0, y0;
  float fx, fy;
  bool gx_on, gy_on;
  if (!warp_coord(fl.x, fl.y, px, py, H, W, border, x0, y0, fx, fy, gx_on, gy_on)) return;
  const Corners k = corners(x0, y0, H, W);
  const double gx = fx, gy = fy;
  const float wq[4] = {(float)((1.0 - gy) * (1.0 - gx)), (float)((1.0 - gy) * gx), (float)(gy * (1.0 - gx)), (float)(gy * gx)};
  const int nc = min(8, C - cg * 8);
  for (int e = 0; e < nc; ++e) {
    const long long base = CB8 ? ((long long)n * CG + cg) * HW * 8 + e : ((long long)n * C + cg * 8 + e) * HW;
    const float gv = CB8 ? g[base + (long long)pix * 8] : g[base + pix];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k.ok[q] && wq[q] != 0.f) atomicAdd(dx + base + (CB8 ? (long long)k.off[q] * 8 : (long long)k.off[q]), gv * wq[q]);
  }
}

// dflow gather: one thread per pixel, channels in order
template <bool CB8>
__global__ __launch_bounds__(256) void flow_warp_bwd_dflow_kernel(const float* __restrict__ x, const float* __restrict__ flow,
                                                                  const float* __restrict__ g, float* __restrict__ dflow, int C,
                                                                  int H, int W, int border) {
  const int HW = H * W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int n = blockIdx.z, CG = (C + 7) / 8;
  const int py = pix / W, px = pix - py * W;
  const float2 fl = *(const float2*)(flow + ((long long)n * HW + pix) * 2);
  int x0, y0;
  float fx, fy;
  bool gx_on, gy_on;
  double sx = 0.0, sy = 0.0;
  if (warp_coord(fl.x, fl.y, px, py, H, W, border, x0, y0, fx, fy, gx_on, gy_on)) {
    const Corners k = corners(x0, y0, H, W);
    const double ax = fx, ay = fy;
    for (int c = 0; c < C; ++c) {
      const long long base = CB8 ? ((long long)n * CG + (c >> 3)) * HW * 8 + (c & 7) : ((long long)n * C + c) * HW;
      const int st = CB8 ? 8 : 1;
      const float* src = x + base;
      const double gv = g[base + (long long)pix * st];
      const double v00 = k.ok[0] ? src[(long long)k.off[0] * st] : 0.f, v01 = k.ok[1] ? src[(long long)k.off[1] * st] : 0.f;
      const double v10 = k.ok[2] ? src[(long long)k.off[2] * st] : 0.f, v11 = k.ok[3] ? src[(long long)k.off[3] * st] : 0.f;
      sx += gv * ((1.0 - ay) * (v01 - v00) + ay * (v11 - v10));
      sy += gv * ((1.0 - ax) * (v10 - v00) + ax * (v11 - v01));
    }
    if (!gx_on) sx = 0.0;
    if (!gy_on) sy = 0.0;
  }
  *(float2*)(dflow + ((long long)n * HW + pix) * 2) = make_float2((float)sx, (float)sy);
}

// ------------------------------------------------------------------------------------------------------- SpyNet pieces
__global__ __launch_bounds__(256) void spynet_level_input_kernel(const float* __restrict__ ref, const float* __restrict__ supp,
                                                                 const float* __restrict__ flow_prev, float* __restrict__ out,
                                                                 float* __restrict__ up_out, int H, int W) {
  const long long img = (long long)blockIdx.z * 3 * (H * W);
  level_input_body<1>(ref + img, supp + img, flow_prev, out, up_out, H, W);  // border padding
}

__global__ __launch_bounds__(256) void spynet_preprocess_kernel(const float* x, float* out, long long hw, const Norm3 nm) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int c = blockIdx.y;
  const long long off = ((long long)blockIdx.z * 3 + c) * hw + i;
  out[off] = (x[off] - nm.mean[c]) / nm.stdv[c];
}

__global__ __launch_bounds__(256) void avgpool2x2_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Ho * Wo) return;
  const int y = i / Wo, xx = i - y * Wo;
  const float* s = x + (long long)blockIdx.z * H * W + (long long)(2 * y) * W + 2 * xx;
  const float2 a = *(const float2*)s, b = *(const float2*)(s + W);
  out[(long long)blockIdx.z * Ho * Wo + i] = ((a.x + a.y) + (b.x + b.y)) * 0.25f;
}

int check_warp_args(const char* who, const void* x, const void* flow, int N, int C, int H, int W, int layout, int padding) {
  SR_CHECK_ARG(x && flow, "%s: null x / flow", who);
  SR_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
  SR_CHECK_ARG(layout == SR_FLOW_NCHW || layout == SR_FLOW_CB8, "%s: layout %d is not supported; supported: 0 (NCHW), 1 (CB8)", who,
               layout);
  SR_CHECK_ARG(padding == SR_FLOW_PAD_ZEROS || padding == SR_FLOW_PAD_BORDER,
               "%s: padding %d is not supported; supported: 0 (zeros), 1 (border)", who, padding);
  SR_CHECK_ARG((long long)H * W < (1ll << 28), "%s: image too large for 32-bit plane offsets", who);
  SR_CHECK_ARG(N <= 65535 && (C + 7) / 8 <= 65535, "%s: N and C / 8 must fit the grid (65535)", who);
  SR_CHECK_ARG(((uintptr_t)flow & 7u) == 0, "%s: flow must be 8-byte aligned", who);
  SR_CHECK_ARG(layout == SR_FLOW_NCHW || sr::aligned16(x), "%s: a CB8 tensor must be 16-byte aligned", who);
  return SR_OK;
}

}  // namespace

extern "C" int sr_conv7x7_instance(int cout, int cin) {
  if (cin == 16 && cout == 2) return 2;
  if (cin == 32 && cout == 64) return 1;
  if ((cin == 8 && cout == 32) || (cin == 64 && cout == 32) || (cin == 32 && cout == 16)) return 0;
  return -1;
}

extern "C" size_t sr_conv7x7_packed_floats(int cout, int cin) {
  const int inst = sr_conv7x7_instance(cout, cin);
  if (inst < 0) return 0;
  return (size_t)(conv7x7_weight_floats(cout, cin, inst) + conv7x7_bias_floats(cout, inst));
}

extern "C" int sr_conv7x7_pack_f32(const float* weight, const float* bias, int cout, int cin, float* packed, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int inst = sr_conv7x7_instance(cout, cin);
  SR_CHECK_ARG(inst >= 0, "sr_conv7x7_pack_f32: (cin, cout) = (%d, %d) is not supported; supported: (8, 32), (32, 64), (64, 32), "
               "(32, 16), (16, 2)", cin, cout);
  SR_CHECK_ARG(weight && packed, "sr_conv7x7_pack_f32: null weight / packed");
  SR_CHECK_ARG(sr::aligned16(packed), "sr_conv7x7_pack_f32: packed must be 16-byte aligned");
  const long long wf = conv7x7_weight_floats(cout, cin, inst), total = wf + conv7x7_bias_floats(cout, inst);
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 151, cin, cout, 1, 7, 7, 0.0, 4.0 * (total + 49.0 * cin * cout));
  hipLaunchKernelGGL(conv7x7_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, weight, bias, packed, cout, cin,
                     inst, wf, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_conv7x7_pack_f32 launch");
  return SR_OK;
}

extern "C" int sr_conv7x7_f32(const sr_conv7x7_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_conv7x7_f32: null descriptor");
  const int inst = sr_conv7x7_instance(d->cout, d->cin);
  SR_CHECK_ARG(inst >= 0, "sr_conv7x7_f32: (cin, cout) = (%d, %d) is not supported; supported: (8, 32), (32, 64), (64, 32), "
               "(32, 16), (16, 2)", d->cin, d->cout);
  SR_CHECK_ARG(d->in && d->packed && d->out, "sr_conv7x7_f32: null in / packed / out");
  SR_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0, "sr_conv7x7_f32: bad shape n=%d h=%d w=%d", d->n, d->h, d->w);
  SR_CHECK_ARG(sr::aligned16(d->in) && sr::aligned16(d->packed) && sr::aligned16(d->out) && sr::aligned16(d->res1),
               "sr_conv7x7_f32: pointers must be 16-byte aligned");
  SR_CHECK_ARG(d->in_img_stride % 4 == 0 && d->out_img_stride % 4 == 0 && d->res1_img_stride % 4 == 0,
               "sr_conv7x7_f32: image strides must be multiples of 4 floats");
  SR_CHECK_ARG(d->relu == 0 || d->relu == 1, "sr_conv7x7_f32: relu must be 0 or 1");
  const long long hw = (long long)d->h * d->w;
  const int cinb = d->cin / 8, coutb = (d->cout + 7) / 8;
  SR_CHECK_ARG(hw * 32 * (cinb > coutb ? cinb : coutb) < (1ll << 31), "sr_conv7x7_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(d->in_img_stride >= hw * 8 * cinb && d->out_img_stride >= hw * 8 * coutb && (!d->res1 || d->res1_img_stride >= hw * 8 * coutb),
               "sr_conv7x7_f32: an image stride is smaller than the image");
  C7Params p = {};
  p.in = d->in;
  p.w = d->packed;
  p.bias = d->packed + conv7x7_weight_floats(d->cout, d->cin, inst);
  p.out = d->out;
  p.res1 = d->res1;
  p.in_ns = d->in_img_stride;
  p.out_ns = d->out_img_stride;
  p.res1_ns = d->res1_img_stride;
  p.cin_blocks = cinb;
  p.cout_blocks = coutb;
  p.cout = d->cout;
  p.H = d->h;
  p.W = d->w;
  p.relu = d->relu;
  const int th = inst == 1 ? 8 : 16;
  p.tiles_x = sr::cdiv(d->w, 32);
  p.tiles_y = sr::cdiv(d->h, th);
  SR_CHECK_ARG((long long)p.tiles_x * p.tiles_y * d->n < (1ll << 31), "sr_conv7x7_f32: grid too large");
  const void* kern = inst == 0 ? (const void*)conv7x7_f32_kernel<1, 4> : inst == 1 ? (const void*)conv7x7_f32_kernel<2, 2>
                                                                                     : (const void*)conv7x7_fewcout_f32_kernel;
  const int lds = inst == 0 ? conv_lds_bytes<1, 4>() : inst == 1 ? conv_lds_bytes<2, 2>() : kFewLds;
  if (int rc = sr::ensure_dynamic_lds(kern, lds)) return rc;
  const dim3 grid((unsigned)(p.tiles_x * p.tiles_y * d->n), 1);
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * (double)hw;
    sr::prof_rec(stream, 148 + inst, d->cin, d->cout, d->n, d->h, d->w, 2.0 * 49.0 * d->cin * d->cout * px,
             4.0 * px * (d->cin + coutb * 8.0 * (d->res1 ? 2 : 1)));
  }
  if (inst == 0)
    hipLaunchKernelGGL((conv7x7_f32_kernel<1, 4>), grid, dim3(256), lds, stream, p);
  else if (inst == 1)
    hipLaunchKernelGGL((conv7x7_f32_kernel<2, 2>), grid, dim3(256), lds, stream, p);
  else
    hipLaunchKernelGGL(conv7x7_fewcout_f32_kernel, grid, dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_conv7x7_f32 launch");
  return SR_OK;
}

extern "C" int sr_flow_warp_f32(const float* x, const float* flow, float* out, int N, int C, int H, int W, int layout, int padding,
                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_warp_args("sr_flow_warp_f32", x, flow, N, C, H, W, layout, padding)) return rc;
  SR_CHECK_ARG(out != nullptr, "sr_flow_warp_f32: null out");
  SR_CHECK_ARG(layout == SR_FLOW_NCHW || sr::aligned16(out), "sr_flow_warp_f32: a CB8 tensor must be 16-byte aligned");
  const dim3 grid((unsigned)sr::cdiv(H * W, 256), (unsigned)((C + 7) / 8), (unsigned)N);
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 152, C, C, N, H, W, 8.0 * N * C * H * W, 4.0 * N * H * W * (5.0 * C + 2.0));
  if (layout == SR_FLOW_CB8)
    hipLaunchKernelGGL(flow_warp_kernel<true>, grid, dim3(256), 0, stream, x, flow, out, C, H, W, padding);
  else
    hipLaunchKernelGGL(flow_warp_kernel<false>, grid, dim3(256), 0, stream, x, flow, out, C, H, W, padding);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_flow_warp_f32 launch");
  return SR_OK;
}

extern "C" int sr_flow_warp_bwd_f32(const float* x, const float* flow, const float* g, float* dx, float* dflow, int N, int C, int H,
                                    int W, int layout, int padding, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_warp_args("sr_flow_warp_bwd_f32", x, flow, N, C, H, W, layout, padding)) return rc;
  SR_CHECK_ARG(g != nullptr, "sr_flow_warp_bwd_f32: null g");
  SR_CHECK_ARG(!dflow || ((uintptr_t)dflow & 7u) == 0, "sr_flow_warp_bwd_f32: dflow must be 8-byte aligned");
  const bool prof = sr::prof_on();
  if (dx) {
    const dim3 grid((unsigned)sr::cdiv(H * W, 256), (unsigned)((C + 7) / 8), (unsigned)N);
    if (prof) sr::prof_rec(stream, 153, C, C, N, H, W, 8.0 * N * C * H * W, 4.0 * N * H * W * (5.0 * C + 2.0));
    if (layout == SR_FLOW_CB8)
      hipLaunchKernelGGL(flow_warp_bwd_dx_kernel<true>, grid, dim3(256), 0, stream, flow, g, dx, C, H, W, padding);
    else
      hipLaunchKernelGGL(flow_warp_bwd_dx_kernel<false>, grid, dim3(256), 0, stream, flow, g, dx, C, H, W, padding);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_flow_warp_bwd_f32 dx launch");
  }
  if (dflow) {
    const dim3 grid((unsigned)sr::cdiv(H * W, 256), 1, (unsigned)N);
    if (prof) sr::prof_rec(stream, 154, C, 2, N, H, W, 14.0 * N * C * H * W, 4.0 * N * H * W * (5.0 * C + 4.0));
    if (layout == SR_FLOW_CB8)
      hipLaunchKernelGGL(flow_warp_bwd_dflow_kernel<true>, grid, dim3(256), 0, stream, x, flow, g, dflow, C, H, W, padding);
    else
      hipLaunchKernelGGL(flow_warp_bwd_dflow_kernel<false>, grid, dim3(256), 0, stream, x, flow, g, dflow, C, H, W, padding);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH("sr_flow_warp_bwd_f32 dflow launch");
  }
  return SR_OK;
}

extern "C" int sr_spynet_level_input_f32(const float* ref, const float* supp, const float* flow_prev, float* out, float* up_out, int N,
                                         int H, int W, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(ref && supp && out && up_out, "sr_spynet_level_input_f32: null ref / supp / out / up_out");
  SR_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0, "sr_spynet_level_input_f32: bad shape N=%d H=%d W=%d", N, H, W);
  SR_CHECK_ARG(!flow_prev || (H % 2 == 0 && W % 2 == 0), "sr_spynet_level_input_f32: H=%d, W=%d must be even above the coarsest level",
               H, W);
  SR_CHECK_ARG((long long)H * W < (1ll << 28), "sr_spynet_level_input_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(sr::aligned16(out) && sr::aligned16(up_out) && sr::aligned16(flow_prev),
               "sr_spynet_level_input_f32: CB8 tensors must be 16-byte aligned");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 155, 8, 8, N, H, W, 40.0 * N * H * W, 4.0 * N * H * W * (3.0 + 12.0 + 2.0 + 16.0));
  hipLaunchKernelGGL(spynet_level_input_kernel, dim3((unsigned)sr::cdiv(H * W, 256), 1, (unsigned)N), dim3(256), 0, stream, ref, supp,
                     flow_prev, out, up_out, H, W);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_spynet_level_input_f32 launch");
  return SR_OK;
}

extern "C" int sr_spynet_preprocess_f32(const float* x, float* out, int N, int H, int W, const float* mean3, const float* std3,
                                        void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && out && mean3 && std3, "sr_spynet_preprocess_f32: null x / out / mean3 / std3");
  SR_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0, "sr_spynet_preprocess_f32: bad shape N=%d H=%d W=%d", N, H, W);
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    SR_CHECK_ARG(std3[c] != 0.f, "sr_spynet_preprocess_f32: std3[%d] is 0", c);
    nm.mean[c] = mean3[c];
    nm.stdv[c] = std3[c];
  }
  const long long hw = (long long)H * W;
  SR_CHECK_ARG(hw < (1ll << 31), "sr_spynet_preprocess_f32: image too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 156, 3, 3, N, H, W, 6.0 * N * hw, 24.0 * N * hw);
  hipLaunchKernelGGL(spynet_preprocess_kernel, dim3((unsigned)((hw + 255) / 256), 3, (unsigned)N), dim3(256), 0, stream, x, out, hw, nm);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_spynet_preprocess_f32 launch");
  return SR_OK;
}

extern "C" int sr_avgpool2x2_f32(const float* x, float* out, int planes, int H, int W, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && out, "sr_avgpool2x2_f32: null x / out");
  SR_CHECK_ARG(planes > 0 && planes <= 65535 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0,
               "sr_avgpool2x2_f32: needs 1..65535 planes of even H x W, got %d of %d x %d", planes, H, W);
  SR_CHECK_ARG((long long)H * W < (1ll << 31), "sr_avgpool2x2_f32: image too large");
  SR_CHECK_ARG(((uintptr_t)x & 7u) == 0, "sr_avgpool2x2_f32: x must be 8-byte aligned");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 157, 1, 1, planes, H / 2, W / 2, 1.0 * planes * H * W, 5.0 * planes * H * W);
  hipLaunchKernelGGL(avgpool2x2_kernel, dim3((unsigned)sr::cdiv((H / 2) * (W / 2), 256), 1, (unsigned)planes), dim3(256), 0, stream, x,
                     out, H, W);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_avgpool2x2_f32 launch");
  return SR_OK;
}
