// Modulated deformable convolution (DCNv2; basicsr/ops/dcn of the reference) on fp32 MFMA for gfx950 (include/sr_hip_dcn.h).
//
// Forward: the implicit GEMM of ridnet_ops.hip's convd_f32_kernel (D[cout][pixel] += W[cout][k] * X[k][pixel] on
// v_mfma_f32_32x32x2_f32, CB8 layout, the same weight image, LDS-DMA weight staging and LDS bank swizzle) whose X operand is
// not a halo'd tile copy but a column image built in LDS by a sampler: per tap, the masked bilinear value of the chunk's 8
// channels (one 32-byte pixel: two 16-byte loads per corner).  Samples may lie anywhere in the image, so nothing is assumed
// about a halo; every corner is checked against the image.
//
// LDS: column image [9 taps][4*PT rows][32][8] fp32 = 36 KiB (PT 1) / 72 KiB (PT 2), single-buffered, plus two weight units
// of 9*COT KiB: 54 .. 108 KiB of the 160 KiB.  A double-buffered 8-row column image (2 x (72 + 18) KiB) does not fit; the
// sampler of one workgroup overlaps the MFMA loop of the other where two fit a CU (PT 1).
//
// Backward: the columns as a CB8 tensor (tap-major) for the ksize-1 weight gradient, the transposed ksize-1 weight image for
// dcol = Wt * dy, and one kernel for doffset / dmask (gather, fixed order) and dx (atomicAdd scatter).
#include <algorithm>

#include "dcn_device.h"
#include "sr_internal.h"
#include "../../include/sr_hip_dcn.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

struct DcnParams {
  const float* x;
  const float* off;
  const float* msk;
  const float* w;
  const float* bias;
  float* out;
  long long x_ns, off_ns, msk_ns, out_ns;
  int cin_blocks, cout_blocks, bpg;  // bpg = CB8 blocks per deformable group
  int H, W;
  int tiles_x, tiles_y;
  int logit;
  float slope;
};

using dcndev::Bilinear;
using dcndev::channel_at;
using dcndev::mask_value;
using dcndev::tap_position;

// Four channels (16 bytes at `xc`, the block's plane offset by the half) of the bilinear value, unmasked.
__device__ __forceinline__ f32x4 sample4(const float* xc, int W, const Bilinear& b) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const float* p = xc + ((long long)b.hl * W + b.wl) * 8;
  const f32x4 a1 = b.v1 ? *(const f32x4*)p : z;
  const f32x4 a2 = b.v2 ? *(const f32x4*)(p + 8) : z;
  const f32x4 a3 = b.v3 ? *(const f32x4*)(p + (long long)W * 8) : z;
  const f32x4 a4 = b.v4 ? *(const f32x4*)(p + (long long)W * 8 + 8) : z;
  const float w1 = b.hh * b.hw, w2 = b.hh * b.lw, w3 = b.lh * b.hw, w4 = b.lh * b.lw;
  return w1 * a1 + w2 * a2 + w3 * a3 + w4 * a4;
}

// One 32-column x (4*PT)-row x (32*COT)-cout tile per workgroup of 4 waves.
template <int COT, int PT>
__global__ __launch_bounds__(256) void dcn_fwd_f32_kernel(const DcnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = 4, TH = NW * PT, NPIX = TH * 32;
  constexpr int CBYTES = 9 * NPIX * 32;  // column image
  constexpr int NWU = 9 * COT, WBYTES = NWU * 1024;
  constexpr int NWR = (NWU + NW - 1) / NW;
  constexpr int W_CHUNK = WBYTES / 4;      // floats of one channel block's weight image
  constexpr int ITEMS = 9 * NPIX * 2 / 256;  // 16-byte sampler items per thread and chunk

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
  const long long HW = (long long)p.H * p.W;
  const float* x_n = p.x + (long long)n * p.x_ns;
  const float* off_n = p.off + (long long)n * p.off_ns;
  const float* msk_n = p.msk + (long long)n * p.msk_ns;
  const float* wg = p.w + (size_t)cog * p.cin_blocks * W_CHUNK;

  const __amdgpu_buffer_rsrc_t w_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)wg, 0, (unsigned)((long long)p.cin_blocks * W_CHUNK * 4), 0x00020000);
  const unsigned wvo = (lane ^ ((lane >> 4) & 1)) * 16;
  char* cols = smem;
  auto stage_w = [&](int buf, int cb) {
    char* ws = smem + CBYTES + buf * WBYTES;
    const unsigned wso = (unsigned)cb * (unsigned)W_CHUNK * 4u;
#pragma unroll
    for (int r = 0; r < NWR; ++r) {
      const int u = r * NW + wave;  // unit = tap * COT + cout sub-tile
      if (u < NWU) sr::blds16(w_rs, wvo, wso + (unsigned)(u * 256) * 4u, ws + u * 1024);
    }
  };

  // The sampler: item q of a chunk = (tap, tile pixel, 16-byte half); the two halves of a pixel are neighbouring lanes.
  auto sample = [&](int cb) {
    const int g = cb / p.bpg;
    const float* xc = x_n + (long long)cb * HW * 8;
#pragma unroll 3
    for (int it = 0; it < ITEMS; ++it) {
      const int q = it * 256 + tid;
      const int half = q & 1, pp = (q >> 1) % NPIX, tap = (q >> 1) / NPIX;
      const int row = pp >> 5, col = pp & 31;
      const int y = y0 + row, x = x0 + col;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (y < p.H && x < p.W) {
        const long long pix = (long long)y * p.W + x;
        const int oc = 18 * g + 2 * tap;
        const float oh = channel_at(off_n, HW, pix, oc), ow = channel_at(off_n, HW, pix, oc + 1);
        const float m = mask_value(channel_at(msk_n, HW, pix, 9 * g + tap), p.logit);
        const Bilinear b = tap_position(y, x, tap, oh, ow, p.H, p.W);
        v = sample4(xc + half * 4, p.W, b) * m;
      }
      *(f32x4*)(cols + ((tap * TH + row) * 32 + col) * 32 + ((half ^ ((col >> 3) & 1)) * 16)) = v;
    }
  };

  f32x16 acc[COT][PT];
#pragma unroll
  for (int a = 0; a < COT; ++a)
#pragma unroll
    for (int b = 0; b < PT; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int xlane = (wave * PT * 32 + j) * 32 + ((h ^ ((j >> 3) & 1)) * 16);
  const int wlane = j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  auto compute = [&](int buf) {
    const char* xb = cols + xlane;
    const char* ws = smem + CBYTES + buf * WBYTES + wlane;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      f32x4 a[COT], b[PT];
#pragma unroll
      for (int c = 0; c < COT; ++c) a[c] = *(const f32x4*)(ws + (tap * COT + c) * 1024);
#pragma unroll
      for (int r = 0; r < PT; ++r) b[r] = *(const f32x4*)(xb + (tap * TH + r) * 1024);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int c = 0; c < COT; ++c)
#pragma unroll
          for (int r = 0; r < PT; ++r)
            acc[c][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][s], b[r][s], acc[c][r], 0, 0, 0);
    }
  };

  const int nchunk = p.cin_blocks;
  stage_w(0, 0);
  for (int c = 0; c < nchunk; ++c) {
    sample(c);
    __syncthreads();  // the column image of chunk c is written and its weight unit has arrived
    if (c + 1 < nchunk) stage_w((c + 1) & 1, c + 1);
    compute(c & 1);
    __syncthreads();
  }

  // epilogue: bias, LeakyReLU
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
        if (p.bias) v += *(const f32x4*)(p.bias + cb * 8 + h * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
        *(f32x4*)(p.out + (long long)n * p.out_ns + (cb * HW + pixoff) * 8 + h * 4) = v;
      }
    }
  }
}

template <int COT, int PT>
constexpr int dcn_lds_bytes() {
  return 9 * 4 * PT * 32 * 32 + 2 * 9 * COT * 1024;
}

// The masked columns, tap-major: one 16-byte half pixel per thread; cols[n][tap * cin_blocks + cb][y][x][8].
__global__ __launch_bounds__(256) void dcn_cols_kernel(const DcnParams p, float* __restrict__ cols, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long HW = (long long)p.H * p.W;
  const int half = (int)(i & 1);
  long long r = i >> 1;
  const long long pix = r % HW;
  r /= HW;
  const int cb = (int)(r % p.cin_blocks);
  r /= p.cin_blocks;
  const int tap = (int)(r % 9);
  const long long n = r / 9;
  const int y = (int)(pix / p.W), x = (int)(pix - (long long)y * p.W);
  const int g = cb / p.bpg;
  const float* off_n = p.off + n * p.off_ns;
  const float* msk_n = p.msk + n * p.msk_ns;
  const int oc = 18 * g + 2 * tap;
  const float oh = channel_at(off_n, HW, pix, oc), ow = channel_at(off_n, HW, pix, oc + 1);
  const float m = mask_value(channel_at(msk_n, HW, pix, 9 * g + tap), p.logit);
  const Bilinear b = tap_position(y, x, tap, oh, ow, p.H, p.W);
  const f32x4 v = sample4(p.x + n * p.x_ns + (long long)cb * HW * 8 + half * 4, p.W, b) * m;
  *(f32x4*)(cols + ((n * 9 * p.cin_blocks + (long long)tap * p.cin_blocks + cb) * HW + pix) * 8 + half * 4) = v;
}

struct DcnBwdParams {
  DcnParams f;
  const float* dcol;
  float* dx;
  float* doff;
  float* dmsk;
  long long dx_ns, doff_ns, dmsk_ns;
  int dg;
};

// One thread per (image, deformable group, tap, pixel): its cpg channels in channel order.
//   dmask   = sum_c dcol_c * sample_c                    (times m (1 - m) for a logit mask)
//   doffset = sum_c (dcol_c * m) * d sample_c / d(h, w)   (dmcn_get_coordinate_weight, deform_conv_cuda_kernel.cu:526-568)
//   dx     += corner weight * (dcol_c * m) at each valid corner (dmcn_get_gradient_weight, :499-524), by atomicAdd
__global__ __launch_bounds__(256) void dcn_bwd_data_kernel(const DcnBwdParams q, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const DcnParams& p = q.f;
  const long long HW = (long long)p.H * p.W;
  long long r = i;
  const long long pix = r % HW;
  r /= HW;
  const int tap = (int)(r % 9);
  r /= 9;
  const int g = (int)(r % q.dg);
  const long long n = r / q.dg;
  const int y = (int)(pix / p.W), x = (int)(pix - (long long)y * p.W);
  const float* off_n = p.off + n * p.off_ns;
  const float* msk_n = p.msk + n * p.msk_ns;
  const int oc = 18 * g + 2 * tap, mc = 9 * g + tap;
  const float oh = channel_at(off_n, HW, pix, oc), ow = channel_at(off_n, HW, pix, oc + 1);
  const float m = mask_value(channel_at(msk_n, HW, pix, mc), p.logit);
  const Bilinear b = tap_position(y, x, tap, oh, ow, p.H, p.W);
  const float w1 = b.hh * b.hw, w2 = b.hh * b.lw, w3 = b.lh * b.hw, w4 = b.lh * b.lw;
  const long long corner = ((long long)b.hl * p.W + b.wl) * 8, down = (long long)p.W * 8;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  float mval = 0.f, dh = 0.f, dw = 0.f;
  for (int blk = 0; blk < p.bpg; ++blk) {
    const int cb = g * p.bpg + blk;
    const float* dc = q.dcol + ((n * 9 * p.cin_blocks + (long long)tap * p.cin_blocks + cb) * HW + pix) * 8;
    const long long plane = n * p.x_ns + (long long)cb * HW * 8 + corner;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const f32x4 d = *(const f32x4*)(dc + half * 4);
      const float* xp = p.x + plane + half * 4;
      const f32x4 a1 = b.v1 ? *(const f32x4*)xp : z;
      const f32x4 a2 = b.v2 ? *(const f32x4*)(xp + 8) : z;
      const f32x4 a3 = b.v3 ? *(const f32x4*)(xp + down) : z;
      const f32x4 a4 = b.v4 ? *(const f32x4*)(xp + down + 8) : z;
      const f32x4 s = w1 * a1 + w2 * a2 + w3 * a3 + w4 * a4;
      const f32x4 ch = b.hw * a3 + b.lw * a4 - b.hw * a1 - b.lw * a2;  // d sample / d h_im
      const f32x4 cw = b.hh * a2 + b.lh * a4 - b.hh * a1 - b.lh * a3;  // d sample / d w_im
      const f32x4 dm = d * m;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        mval += d[e] * s[e];
        dh += ch[e] * dm[e];
        dw += cw[e] * dm[e];
      }
      if (q.dx) {
        float* o = q.dx + n * q.dx_ns + (long long)cb * HW * 8 + corner + half * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (b.v1) atomicAdd(o + e, w1 * dm[e]);
          if (b.v2) atomicAdd(o + 8 + e, w2 * dm[e]);
          if (b.v3) atomicAdd(o + down + e, w3 * dm[e]);
          if (b.v4) atomicAdd(o + down + 8 + e, w4 * dm[e]);
        }
      }
    }
  }
  if (q.doff) {
    float* o = q.doff + n * q.doff_ns;
    o[((long long)(oc >> 3) * HW + pix) * 8 + (oc & 7)] = dh;
    o[((long long)((oc + 1) >> 3) * HW + pix) * 8 + ((oc + 1) & 7)] = dw;
    q.dmsk[n * q.dmsk_ns + ((long long)(mc >> 3) * HW + pix) * 8 + (mc & 7)] = p.logit ? mval * (m * (1.f - m)) : mval;
  }
}

// OIHW [cout][cin][3][3] -> the ksize-1 forward image wp[o / gc][co >> 3][o % gc][co & 7] of Wt[o = tap * cin + ci][co]
__global__ void dcn_pack_t_kernel(const float* __restrict__ w, int cout, int cin, float* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cout * cin * 9) return;
  const int tap = i % 9, ci = (i / 9) % cin, co = i / (9 * cin);
  const int o = tap * cin + ci, gc = sr::group_couts(9 * cin), cbs = (cout + 7) / 8;
  wp[(((long long)(o / gc) * cbs + (co >> 3)) * gc + o % gc) * 8 + (co & 7)] = w[i];
}

__global__ void dcn_weight_unpack_kernel(const float* __restrict__ dwc, int cout, int cin, float* __restrict__ dw, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cout * cin * 9) return;
  const int tap = i % 9, ci = (i / 9) % cin, co = i / (9 * cin);
  const float v = dwc[(long long)co * 9 * cin + tap * cin + ci];
  dw[i] = accumulate ? dw[i] + v : v;
}

int check_desc(const sr_dcn_desc* d, const char* who, bool need_weights) {
  SR_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  SR_CHECK_ARG(d->ksize == 3 && d->stride == 1 && d->padding == 1 && d->dilation == 1 && d->groups == 1,
               "%s: kernel %d stride %d padding %d dilation %d groups %d not supported (3x3, stride 1, padding 1, dilation 1, groups 1 "
               "only)",
               who, d->ksize, d->stride, d->padding, d->dilation, d->groups);
  SR_CHECK_ARG(d->x && d->offset && d->mask, "%s: null x / offset / mask", who);
  SR_CHECK_ARG(d->n > 0 && d->cin > 0 && d->cout > 0 && d->h > 0 && d->w > 0 && d->deformable_groups > 0, "%s: bad shape", who);
  SR_CHECK_ARG(d->cin % d->deformable_groups == 0 && (d->cin / d->deformable_groups) % 8 == 0,
               "%s: cin %d / deformable_groups %d must be a multiple of 8 (a CB8 block never straddles two groups)", who, d->cin,
               d->deformable_groups);
  SR_CHECK_ARG(((uintptr_t)d->x | (uintptr_t)d->offset | (uintptr_t)d->mask | (uintptr_t)d->wpacked | (uintptr_t)d->bpacked |
                (uintptr_t)d->out) % 16 == 0 &&
                   (d->x_img_stride | d->offset_img_stride | d->mask_img_stride | d->out_img_stride) % 4 == 0,
               "%s: pointers must be 16-byte aligned", who);
  if (need_weights) SR_CHECK_ARG(d->wpacked && d->out, "%s: null wpacked / out", who);
  const long long blocks = std::max({9ll * d->cin / 8, (long long)(d->cout + 7) / 8, (18ll * d->deformable_groups + 7) / 8});
  SR_CHECK_ARG((long long)d->h * d->w * 8 * blocks * 4 < (1ll << 32), "%s: image too large", who);
  return SR_OK;
}

DcnParams params_of(const sr_dcn_desc* d) {
  DcnParams p = {};
  p.x = d->x;
  p.off = d->offset;
  p.msk = d->mask;
  p.w = d->wpacked;
  p.bias = d->bpacked;
  p.out = d->out;
  p.x_ns = d->x_img_stride;
  p.off_ns = d->offset_img_stride;
  p.msk_ns = d->mask_img_stride;
  p.out_ns = d->out_img_stride;
  p.cin_blocks = d->cin / 8;
  p.cout_blocks = (d->cout + 7) / 8;
  p.bpg = d->cin / d->deformable_groups / 8;
  p.H = d->h;
  p.W = d->w;
  p.tiles_x = sr::cdiv(d->w, 32);
  p.logit = d->mask_is_logit;
  p.slope = d->act_slope;
  return p;
}

void prof_dcn(hipStream_t stream, int id, const sr_dcn_desc* d, double flops, double bytes) {
  sr_launch_record r = {};
  r.kernel_id = id;
  r.cin = d->cin;
  r.cout = d->cout;
  r.n = d->n;
  r.h = d->h;
  r.w = d->w;
  r.flops = flops;
  r.bytes = bytes;
  sr::prof_begin(stream, r);
}

template <int COT, int PT>
int dcn_launch(const DcnParams& p, int groups, const sr_dcn_desc* d, hipStream_t stream) {
  constexpr int lds = dcn_lds_bytes<COT, PT>();
  auto kern = dcn_fwd_f32_kernel<COT, PT>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, lds)) return rc;
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * d->h * d->w;
    prof_dcn(stream, 110, d, 2.0 * 9 * d->cin * d->cout * px, 4.0 * px * (d->cin + d->cout + 27 * d->deformable_groups));
  }
  hipLaunchKernelGGL(kern, dim3(p.tiles_x * p.tiles_y * d->n, groups), dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("dcn_fwd_f32 launch");
  return SR_OK;
}

}  // namespace

extern "C" int sr_dcn_fwd_f32(const sr_dcn_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_desc(d, "sr_dcn_fwd_f32", true)) return rc;
  DcnParams p = params_of(d);
  const int gc = sr::group_couts(d->cout);
  const int groups = ((d->cout + 31) / 32 * 32) / gc;
  SR_CHECK_ARG((long long)p.tiles_x * sr::cdiv(p.H, 4) * d->n < (1ll << 31), "sr_dcn_fwd_f32: grid too large");
  // 8-row tiles; 4-row tiles when the launch would not cover the chip once (as sr_convd_f32)
  p.tiles_y = sr::cdiv(p.H, 8);
  const bool small = (long long)p.tiles_x * p.tiles_y * d->n * groups < 256 && p.H > 4;
  if (small) p.tiles_y = sr::cdiv(p.H, 4);
  if (gc == 64) return small ? dcn_launch<2, 1>(p, groups, d, stream) : dcn_launch<2, 2>(p, groups, d, stream);
  return small ? dcn_launch<1, 1>(p, groups, d, stream) : dcn_launch<1, 2>(p, groups, d, stream);
}

extern "C" size_t sr_dcn_cols_bytes(int n, int cin, int h, int w) {
  if (n <= 0 || cin <= 0 || cin % 8 || h <= 0 || w <= 0) return 0;
  return (size_t)n * 9 * cin * h * w * sizeof(float);
}

extern "C" int sr_dcn_cols_f32(const sr_dcn_desc* d, float* cols, size_t cols_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_desc(d, "sr_dcn_cols_f32", false)) return rc;
  SR_CHECK_ARG(cols && (uintptr_t)cols % 16 == 0, "sr_dcn_cols_f32: cols must be non-null and 16-byte aligned");
  const size_t need = sr_dcn_cols_bytes(d->n, d->cin, d->h, d->w);
  if (cols_bytes < need) {
    sr::set_error("sr_dcn_cols_f32: cols %zu B too small (need %zu B)", cols_bytes, need);
    return SR_ENOSPACE;
  }
  const DcnParams p = params_of(d);
  const long long total = (long long)d->n * 9 * p.cin_blocks * d->h * d->w * 2;
  SR_CHECK_ARG((total + 255) / 256 < (1ll << 31), "sr_dcn_cols_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * d->h * d->w;
    prof_dcn(stream, 111, d, 9.0 * 8 * d->cin * px, 4.0 * px * (d->cin + 9 * d->cin + 27 * d->deformable_groups));
  }
  hipLaunchKernelGGL(dcn_cols_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p, cols, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("dcn_cols launch");
  return SR_OK;
}

extern "C" size_t sr_dcn_packed_t_weight_floats(int cout, int cin) {
  if (cout <= 0 || cin <= 0) return 0;
  return (size_t)((9 * cin + 31) / 32 * 32) * ((cout + 7) / 8 * 8);
}

extern "C" int sr_dcn_pack_t_f32(const float* weight, int cout, int cin, float* wpacked, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(weight && wpacked && cout > 0 && cin > 0 && cin % 8 == 0, "sr_dcn_pack_t_f32: bad argument");
  if (hipMemsetAsync(wpacked, 0, sr_dcn_packed_t_weight_floats(cout, cin) * sizeof(float), stream) != hipSuccess) {
    sr::set_error("sr_dcn_pack_t_f32: memset failed");
    return SR_ELAUNCH;
  }
  const int total = cout * cin * 9;
  hipLaunchKernelGGL(dcn_pack_t_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, weight, cout, cin, wpacked);
  SR_CHECK_LAUNCH("dcn_pack_t");
  return SR_OK;
}

extern "C" int sr_dcn_weight_unpack_f32(const float* dw_cols, int cout, int cin, float* dweight, int accumulate, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(dw_cols && dweight && cout > 0 && cin > 0, "sr_dcn_weight_unpack_f32: bad argument");
  const int total = cout * cin * 9;
  hipLaunchKernelGGL(dcn_weight_unpack_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, dw_cols, cout, cin, dweight, accumulate);
  SR_CHECK_LAUNCH("dcn_weight_unpack");
  return SR_OK;
}

extern "C" int sr_dcn_bwd_data_f32(const sr_dcn_bwd_desc* dd, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(dd != nullptr, "sr_dcn_bwd_data_f32: null descriptor");
  const sr_dcn_desc* d = &dd->fwd;
  if (int rc = check_desc(d, "sr_dcn_bwd_data_f32", false)) return rc;
  SR_CHECK_ARG(dd->dcol, "sr_dcn_bwd_data_f32: null dcol");
  SR_CHECK_ARG((dd->doffset == nullptr) == (dd->dmask == nullptr), "sr_dcn_bwd_data_f32: doffset and dmask go together");
  SR_CHECK_ARG(((uintptr_t)dd->dcol | (uintptr_t)dd->dx | (uintptr_t)dd->doffset | (uintptr_t)dd->dmask) % 16 == 0,
               "sr_dcn_bwd_data_f32: pointers must be 16-byte aligned");
  if (!dd->dx && !dd->doffset) return SR_OK;
  DcnBwdParams q = {};
  q.f = params_of(d);
  q.dcol = dd->dcol;
  q.dx = dd->dx;
  q.doff = dd->doffset;
  q.dmsk = dd->dmask;
  q.dx_ns = dd->dx_img_stride;
  q.doff_ns = dd->doffset_img_stride;
  q.dmsk_ns = dd->dmask_img_stride;
  q.dg = d->deformable_groups;
  const long long total = (long long)d->n * q.dg * 9 * d->h * d->w;
  SR_CHECK_ARG((total + 255) / 256 < (1ll << 31), "sr_dcn_bwd_data_f32: grid too large");
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * d->h * d->w;
    // bytes: dcol + 4 corners of x per tap + offsets / masks and their gradients + the dx atomics (36 * cin * 4 B per pixel)
    prof_dcn(stream, 112, d, 9.0 * 14 * d->cin * px, 4.0 * px * (9 * d->cin + 36 * d->cin + 54 * q.dg + (dd->dx ? 36 * d->cin : 0)));
  }
  hipLaunchKernelGGL(dcn_bwd_data_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, q, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("dcn_bwd_data launch");
  return SR_OK;
}
