// The pieces of TOFlow on gfx950 (include/sr_hip_tof.h): the 9x9 convolution of the reconstruction module, SPyNetTOF's level
// input, the aligned 7-frame stack and the finish.
//
// Reference: TOFlow (basicsr/archs/tof_arch.py) estimates six flows with SPyNetTOF (four pyramid levels of five 7x7 convs with
// BatchNorm), warps the six neighbours onto the reference frame, and runs conv 9x9 (21 -> 64), conv 9x9 (64 -> 64), two 1x1 convs
// and a residual.  The 7x7 convs run on flow_ops.hip with the BatchNorm folded on the host; the 1x1 convs on ridnet_ops.hip.
//
// 9x9 convolution: the implicit GEMM of conv7x7_body<2, 2> (flow_device.h) with a 9-tap window:  D[cout][pixel] += W[cout][k] *
// X[k][pixel], k = (cin, tap), on v_mfma_f32_32x32x2_f32; A = weights, B = activations, the pixel on the lane and 4 consecutive
// couts in 4 consecutive accumulator registers, so that a quad is one 16-byte store into CB8.  Workgroup = 4 waves, output tile =
// 8 rows x 32 columns x 64 couts; wave w owns rows 2w, 2w + 1.  K = 81 * cin_pad is walked in chunks of (one 8-channel block,
// one TAP ROW): the halo'd X tile [8 + 8][40][8] (20 KiB) is staged once per channel block, the weights [9 taps][64][8] (18 KiB)
// once per chunk, both by LDS-DMA through buffer descriptors (1 KiB per wave-instruction), both double buffered, one barrier per
// chunk: 2 * (20 + 18) KiB = 76 KiB, so two workgroups share a CU's 160 KiB (two waves per SIMD, 64 accumulator registers each).
// The 4-pixel zero padding is the hardware's zero fill of a buffer load beyond num_records: pad lanes carry an offset outside the
// descriptor.  Per chunk and wave: 9 * 4 ds_read_b128 feed 144 MFMAs of 64 cycles.
// The source of conv_1 has 21 channels in 3 blocks: in the last block the lanes that hold channels 21-23 replace what they read
// by zero (three selects per B operand), so those channels may hold anything.
#include <math.h>

#include "../../include/sr_hip_tof.h"
#include "flow_device.h"
#include "sr_internal.h"

using namespace flowdev;  // xcd_tile, the warp rule and the level coordinate, shared with flow_ops.hip

namespace {

void prof_rec(hipStream_t stream, int id, int cin, int cout, int n, int h, int w, double flops, double bytes) {
  sr_launch_record r = {};
  r.kernel_id = id;
  r.cin = cin;
  r.cout = cout;
  r.n = n;
  r.h = h;
  r.w = w;
  r.flops = flops;
  r.bytes = bytes;
  sr::prof_begin(stream, r);
}

// ------------------------------------------------------------------------------------------------------------ conv 9x9
constexpr int k9 = 9, k9Pad = 4, k9Row = 32 + k9 - 1;   // taps, padding, columns of the halo'd tile
constexpr int k9COT = 2, k9PT = 2, k9TH = 4 * k9PT;     // 64 couts, 2 rows per wave, 8 rows per tile
constexpr int k9XPix = (k9TH + k9 - 1) * k9Row;
constexpr int k9XBytes = ((k9XPix * 32 + 1023) / 1024) * 1024, k9NXU = k9XBytes / 1024, k9NXR = (k9NXU + 3) / 4;
constexpr int k9NWU = k9 * k9COT, k9WBytes = k9NWU * 1024, k9NWR = (k9NWU + 3) / 4;
constexpr int k9Lds = 2 * (k9XBytes + k9WBytes);

struct C9Params {
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  long long in_ns, out_ns;
  int cin, cin_blocks, H, W, tiles_x, tiles_y, relu;
};

__global__ __launch_bounds__(256, 2) void tof_conv9x9_f32_kernel(const C9Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  int t = xcd_tile(gridDim.x, blockIdx.x);
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y, n = t / p.tiles_y;
  const int x0 = tx * 32, y0 = ty * k9TH;
  const int HW = p.H * p.W;
  const float* in_n = p.in + (long long)n * p.in_ns;

  // per-lane byte offsets of the X pieces this wave stages (pad lanes: an offset beyond the descriptor, which reads as zero)
  unsigned xvo[k9NXR];
#pragma unroll
  for (int r = 0; r < k9NXR; ++r) {
    const int q = (r * 4 + wave) * 64 + lane;
    const int pix = q >> 1, half = q & 1;
    const int row = pix / k9Row, col = pix - row * k9Row;
    const int gy = y0 - k9Pad + row, gx = x0 - k9Pad + col;
    const bool valid = pix < k9XPix && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
    // LDS bank swizzle, as the 7x7 body: the 16-byte halves of tile column c are stored swapped when bit 3 of c is set
    const int hsw = half ^ ((col >> 3) & 1);
    xvo[r] = valid ? (unsigned)((gy * p.W + gx) * 8 + hsw * 4) * 4u : 0xfffffff0u;
  }
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)in_n, 0, (unsigned)p.cin_blocks * (unsigned)HW * 32u, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (unsigned)p.cin_blocks * (unsigned)(k9 * k9WBytes), 0x00020000);
  const unsigned wvo = (unsigned)(lane ^ ((lane >> 4) & 1)) * 16u;  // unit (cout i, half) <- half ^ bit3(i)
  char* const xs0 = smem;
  char* const ws0 = smem + 2 * k9XBytes;
  auto stage_x = [&](int buf, int cb) {
    char* xs = xs0 + buf * k9XBytes;
    const unsigned so = (unsigned)cb * (unsigned)HW * 32u;
#pragma unroll
    for (int r = 0; r < k9NXR; ++r) {
      const int u = r * 4 + wave;
      if (u < k9NXU) sr::blds16(x_rs, xvo[r], so, xs + u * 1024);
    }
  };
  auto stage_w = [&](int buf, int chunk) {  // chunk = cb * 9 + tap row
    char* ws = ws0 + buf * k9WBytes;
    const unsigned so = (unsigned)chunk * (unsigned)k9WBytes;
#pragma unroll
    for (int r = 0; r < k9NWR; ++r) {
      const int u = r * 4 + wave;  // unit = tap column * 2 + cout sub-tile
      if (u < k9NWU) sr::blds16(w_rs, wvo, so + (unsigned)u * 1024u, ws + u * 1024);
    }
  };

  f32x16 acc[k9COT][k9PT];
#pragma unroll
  for (int a = 0; a < k9COT; ++a)
#pragma unroll
    for (int b = 0; b < k9PT; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int xbase = ((wave * k9PT) * k9Row + j) * 32;  // this lane's pixel at tap (0, 0), row group 0
  const int wlane = j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  // lim: how many of this lane's 4 channels of the block are real (4 everywhere but in the last block of the 21-channel source)
  auto compute = [&](int xbuf, int wbuf, int dy, int lim) {
    const char* xb = xs0 + xbuf * k9XBytes + dy * (k9Row * 32) + xbase;
    const char* ws = ws0 + wbuf * k9WBytes + wlane;
#pragma unroll
    for (int dx = 0; dx < k9; ++dx) {
      f32x4 a[k9COT], b[k9PT];
      const int xo = dx * 32 + ((h ^ (((j + dx) >> 3) & 1)) * 16);  // swizzled half of tile column j + dx
#pragma unroll
      for (int c = 0; c < k9COT; ++c) a[c] = *(const f32x4*)(ws + (dx * k9COT + c) * 1024);
#pragma unroll
      for (int r = 0; r < k9PT; ++r) {
        b[r] = *(const f32x4*)(xb + xo + r * (k9Row * 32));
#pragma unroll
        for (int s = 1; s < 4; ++s) b[r][s] = s < lim ? b[r][s] : 0.f;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int c = 0; c < k9COT; ++c)
#pragma unroll
          for (int r = 0; r < k9PT; ++r) acc[c][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][s], b[r][s], acc[c][r], 0, 0, 0);
    }
  };

  const int nchunk = p.cin_blocks * k9;
  stage_x(0, 0);
  stage_w(0, 0);
  __syncthreads();
  int cb = 0, dy = 0;
  for (int c = 0; c < nchunk; ++c) {
    if (c + 1 < nchunk) stage_w((c + 1) & 1, c + 1);
    if (dy == 0 && cb + 1 < p.cin_blocks) stage_x((cb + 1) & 1, cb + 1);  // that buffer was last read in block cb - 1
    compute(cb & 1, c & 1, dy, p.cin - cb * 8 - h * 4);
    __syncthreads();  // drains the LDS-DMA issued above and frees the buffers just read
    if (++dy == k9) {
      dy = 0;
      ++cb;
    }
  }

  // ---- epilogue: bias, ReLU
  const int x = x0 + j;
#pragma unroll
  for (int r = 0; r < k9PT; ++r) {
    const int y = y0 + wave * k9PT + r;
    if (y >= p.H || x >= p.W) continue;
    const long long pixoff = (long long)y * p.W + x;
#pragma unroll
    for (int c = 0; c < k9COT; ++c) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ob = c * 4 + g;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[c][r][g * 4 + e];
        const long long off = ((long long)ob * HW + pixoff) * 8 + h * 4;
        v += *(const f32x4*)(p.bias + ob * 8 + h * 4);
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        *(f32x4*)(p.out + (long long)n * p.out_ns + off) = v;
      }
    }
  }
}

// Weight image [cin block][tap row][tap column][2][32 couts][8 channels], then the 64 biases.
__global__ __launch_bounds__(256) void tof_conv9x9_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ out, int cout, int cin, long long wfloats,
                                                               long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  if (idx >= wfloats) {
    const int b = (int)(idx - wfloats);
    out[idx] = (bias && b < cout) ? bias[b] : 0.f;
    return;
  }
  const int ch = (int)(idx & 7);
  const int co = (int)((idx >> 3) & 63);  // (cout sub-tile, cout within it)
  const long long rest = idx >> 9;
  const int tap = (int)(rest % 81), cb = (int)(rest / 81);
  const int ci = cb * 8 + ch;
  out[idx] = (co < cout && ci < cin) ? w[((long long)co * cin + ci) * 81 + tap] : 0.f;
}

bool conv9x9_served(int cout, int cin) { return cout == 64 && (cin == 21 || cin == 64); }
long long conv9x9_weight_floats(int cin) { return (long long)((cin + 7) / 8) * 81 * 512; }

// --------------------------------------------------------------------------------------------------------- level input
// spynet_level_input_kernel (flow_ops.hip) with zeros padding and grouped frame addressing; the same expressions in the same order.
__global__ __launch_bounds__(256) void tof_level_input_kernel(const float* __restrict__ ref, long long ref_gs,
                                                              const float* __restrict__ supp, long long supp_gs, int group, int skip,
                                                              const float* __restrict__ flow_prev, float* __restrict__ out,
                                                              float* __restrict__ up_out, int H, int W) {
  const int HW = H * W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int n = blockIdx.z;
  const int py = pix / W, px = pix - py * W;
  float ux = 0.f, uy = 0.f;
  if (flow_prev) {
    const int Hp = H / 2, Wp = W / 2;
    int ya, yb, xa, xb;
    double fy, fx;
    up_coord(py, H, Hp, ya, yb, fy);
    up_coord(px, W, Wp, xa, xb, fx);
    const float* f = flow_prev + (long long)n * Hp * Wp * 8;
    const float2 v00 = *(const float2*)(f + ((long long)ya * Wp + xa) * 8), v01 = *(const float2*)(f + ((long long)ya * Wp + xb) * 8);
    const float2 v10 = *(const float2*)(f + ((long long)yb * Wp + xa) * 8), v11 = *(const float2*)(f + ((long long)yb * Wp + xb) * 8);
    ux = (float)(2.0 * ((1.0 - fy) * ((1.0 - fx) * v00.x + fx * v01.x) + fy * ((1.0 - fx) * v10.x + fx * v11.x)));
    uy = (float)(2.0 * ((1.0 - fy) * ((1.0 - fx) * v00.y + fx * v01.y) + fy * ((1.0 - fx) * v10.y + fx * v11.y)));
  }
  int x0, y0;
  float fx, fy;
  bool gx_on, gy_on;
  const bool any = warp_coord(ux, uy, px, py, H, W, 0, x0, y0, fx, fy, gx_on, gy_on);
  Corners k = {};
  if (any) k = corners(x0, y0, H, W);
  const int g = n / group, kk = n - g * group;
  const float* rimg = ref + (long long)g * ref_gs;
  const float* simg = supp + (long long)g * supp_gs + (long long)(kk + (kk >= skip ? 1 : 0)) * 3 * HW;
  float o[8];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = rimg[(long long)c * HW + pix];
    const float* s = simg + (long long)c * HW;
    float r = 0.f;
    if (any)
      r = blend(k.ok[0] ? s[k.off[0]] : 0.f, k.ok[1] ? s[k.off[1]] : 0.f, k.ok[2] ? s[k.off[2]] : 0.f, k.ok[3] ? s[k.off[3]] : 0.f,
                fx, fy);
    o[3 + c] = r;
  }
  o[6] = ux;
  o[7] = uy;
  float* dst = out + ((long long)n * HW + pix) * 8;
  *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
  *(f32x4*)(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
  float* du = up_out + ((long long)n * HW + pix) * 8;
  *(f32x4*)du = f32x4{ux, uy, 0.f, 0.f};
  *(f32x4*)(du + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ------------------------------------------------------------------------------------------------------- aligned stack
// grid (ceil(hw / 256), 1, b): a thread writes the 24 channels of one pixel
__global__ __launch_bounds__(256) void tof_align_kernel(const float* __restrict__ clip, const float* __restrict__ flows,
                                                        long long flow_ns, float* __restrict__ out, long long out_ns, int ref_idx,
                                                        int H, int W) {
  const int HW = H * W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int n = blockIdx.z;
  const int py = pix / W, px = pix - py * W;
  float o[24];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const float* frame = clip + ((long long)n * 7 + i) * 3 * HW;
    if (i == ref_idx) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[3 * i + c] = frame[(long long)c * HW + pix];
      continue;
    }
    const int kk = i < ref_idx ? i : i - 1;
    const float2 fl = *(const float2*)(flows + ((long long)n * 6 + kk) * flow_ns + (long long)pix * 8);
    int x0, y0;
    float fx, fy;
    bool gx_on, gy_on;
    const bool any = warp_coord(fl.x, fl.y, px, py, H, W, 0, x0, y0, fx, fy, gx_on, gy_on);
    Corners k = {};
    if (any) k = corners(x0, y0, H, W);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* s = frame + (long long)c * HW;
      float r = 0.f;
      if (any)
        r = blend(k.ok[0] ? s[k.off[0]] : 0.f, k.ok[1] ? s[k.off[1]] : 0.f, k.ok[2] ? s[k.off[2]] : 0.f,
                  k.ok[3] ? s[k.off[3]] : 0.f, fx, fy);
      o[3 * i + c] = r;
    }
  }
  o[21] = o[22] = o[23] = 0.f;
  float* dst = out + (long long)n * out_ns + (long long)pix * 8;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    *(f32x4*)(dst + (long long)b * HW * 8) = f32x4{o[8 * b], o[8 * b + 1], o[8 * b + 2], o[8 * b + 3]};
    *(f32x4*)(dst + (long long)b * HW * 8 + 4) = f32x4{o[8 * b + 4], o[8 * b + 5], o[8 * b + 6], o[8 * b + 7]};
  }
}

// -------------------------------------------------------------------------------------------------------------- finish
struct Norm3 {
  float mean[3], stdv[3];
};
__global__ __launch_bounds__(256) void tof_finish_kernel(const float* __restrict__ y, long long y_ns, const float* __restrict__ lr,
                                                         long long lr_ns, float* __restrict__ out, int HW, const Norm3 nm) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int n = blockIdx.z;
  const f32x4 v = *(const f32x4*)(y + (long long)n * y_ns + (long long)pix * 8);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = v[c] + lr[(long long)n * lr_ns + (long long)c * HW + pix];
    out[((long long)n * 3 + c) * HW + pix] = s * nm.stdv[c] + nm.mean[c];
  }
}

}  // namespace

extern "C" size_t sr_tof_conv9x9_packed_floats(int cout, int cin) {
  if (!conv9x9_served(cout, cin)) return 0;
  return (size_t)(conv9x9_weight_floats(cin) + 64);
}

extern "C" int sr_tof_conv9x9_pack_f32(const float* weight, const float* bias, int cout, int cin, float* packed, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(conv9x9_served(cout, cin), "sr_tof_conv9x9_pack_f32: (cin, cout) = (%d, %d) is not supported; supported: (21, 64), (64, 64)",
               cin, cout);
  SR_CHECK_ARG(weight && packed, "sr_tof_conv9x9_pack_f32: null weight / packed");
  SR_CHECK_ARG(sr::aligned16(packed), "sr_tof_conv9x9_pack_f32: packed must be 16-byte aligned");
  const long long wf = conv9x9_weight_floats(cin), total = wf + 64;
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 189, cin, cout, 1, 9, 9, 0.0, 4.0 * (total + 81.0 * cin * cout));
  hipLaunchKernelGGL(tof_conv9x9_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, weight, bias, packed, cout,
                     cin, wf, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_tof_conv9x9_pack_f32 launch");
  return SR_OK;
}

extern "C" int sr_tof_conv9x9_f32(const sr_tof_conv9x9_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_tof_conv9x9_f32: null descriptor");
  SR_CHECK_ARG(conv9x9_served(d->cout, d->cin), "sr_tof_conv9x9_f32: (cin, cout) = (%d, %d) is not supported; supported: (21, 64), (64, 64)",
               d->cin, d->cout);
  SR_CHECK_ARG(d->in && d->packed && d->out, "sr_tof_conv9x9_f32: null in / packed / out");
  SR_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0, "sr_tof_conv9x9_f32: bad shape n=%d h=%d w=%d", d->n, d->h, d->w);
  SR_CHECK_ARG(sr::aligned16(d->in) && sr::aligned16(d->packed) && sr::aligned16(d->out), "sr_tof_conv9x9_f32: pointers must be 16-byte aligned");
  SR_CHECK_ARG(d->in_img_stride % 4 == 0 && d->out_img_stride % 4 == 0, "sr_tof_conv9x9_f32: image strides must be multiples of 4 floats");
  SR_CHECK_ARG(d->relu == 0 || d->relu == 1, "sr_tof_conv9x9_f32: relu must be 0 or 1");
  const long long hw = (long long)d->h * d->w;
  const int cinb = (d->cin + 7) / 8, coutb = d->cout / 8;
  SR_CHECK_ARG(hw < (1ll << 31) / (32 * (cinb > coutb ? cinb : coutb)), "sr_tof_conv9x9_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(d->in_img_stride >= hw * 8 * cinb && d->out_img_stride >= hw * 8 * coutb,
               "sr_tof_conv9x9_f32: an image stride is smaller than the image");
  C9Params p = {};
  p.in = d->in;
  p.w = d->packed;
  p.bias = d->packed + conv9x9_weight_floats(d->cin);
  p.out = d->out;
  p.in_ns = d->in_img_stride;
  p.out_ns = d->out_img_stride;
  p.cin = d->cin;
  p.cin_blocks = cinb;
  p.H = d->h;
  p.W = d->w;
  p.relu = d->relu;
  p.tiles_x = sr::cdiv(d->w, 32);
  p.tiles_y = sr::cdiv(d->h, k9TH);
  SR_CHECK_ARG((long long)p.tiles_x * p.tiles_y * d->n < (1ll << 31), "sr_tof_conv9x9_f32: grid too large");
  if (int rc = sr::ensure_dynamic_lds((const void*)tof_conv9x9_f32_kernel, k9Lds)) return rc;
  const dim3 grid((unsigned)(p.tiles_x * p.tiles_y * d->n), 1);
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * (double)hw;
    prof_rec(stream, 188, d->cin, d->cout, d->n, d->h, d->w, 2.0 * 81.0 * d->cin * d->cout * px, 4.0 * px * (cinb * 8.0 + d->cout));
  }
  hipLaunchKernelGGL(tof_conv9x9_f32_kernel, grid, dim3(256), k9Lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_tof_conv9x9_f32 launch");
  return SR_OK;
}

extern "C" int sr_tof_level_input_f32(const float* ref, long long ref_group_stride, const float* supp, long long supp_group_stride,
                                      int group, int skip, const float* flow_prev, float* out, float* up_out, int N, int H, int W,
                                      void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(ref && supp && out && up_out, "sr_tof_level_input_f32: null ref / supp / out / up_out");
  SR_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0, "sr_tof_level_input_f32: bad shape N=%d H=%d W=%d", N, H, W);
  SR_CHECK_ARG(group > 0 && N % group == 0 && skip >= 0 && skip <= group,
               "sr_tof_level_input_f32: N=%d must be a multiple of group=%d > 0, and skip=%d within 0..group", N, group, skip);
  SR_CHECK_ARG(!flow_prev || (H % 2 == 0 && W % 2 == 0), "sr_tof_level_input_f32: H=%d, W=%d must be even above the coarsest level", H, W);
  SR_CHECK_ARG((long long)H * W < (1ll << 28), "sr_tof_level_input_f32: image too large for 32-bit plane offsets");
  const long long hw3 = 3ll * H * W;
  SR_CHECK_ARG(ref_group_stride >= hw3 && supp_group_stride >= hw3 * (group + (skip < group ? 1 : 0)),
               "sr_tof_level_input_f32: a group stride is smaller than the frames of a group");
  SR_CHECK_ARG(sr::aligned16(out) && sr::aligned16(up_out) && sr::aligned16(flow_prev),
               "sr_tof_level_input_f32: CB8 tensors must be 16-byte aligned");
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 190, 8, 8, N, H, W, 40.0 * N * H * W, 4.0 * N * H * W * (3.0 + 12.0 + 2.0 + 16.0));
  hipLaunchKernelGGL(tof_level_input_kernel, dim3((unsigned)sr::cdiv(H * W, 256), 1, (unsigned)N), dim3(256), 0, stream, ref,
                     ref_group_stride, supp, supp_group_stride, group, skip, flow_prev, out, up_out, H, W);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_tof_level_input_f32 launch");
  return SR_OK;
}

extern "C" int sr_tof_align_f32(const float* clip, const float* flows, long long flow_img_stride, float* out, long long out_img_stride,
                                int b, int ref_idx, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(clip && flows && out, "sr_tof_align_f32: null clip / flows / out");
  SR_CHECK_ARG(b > 0 && b <= 65535 && h > 0 && w > 0, "sr_tof_align_f32: bad shape b=%d h=%d w=%d", b, h, w);
  SR_CHECK_ARG(ref_idx >= 0 && ref_idx < 7, "sr_tof_align_f32: ref_idx %d is not one of the 7 frames", ref_idx);
  const long long hw = (long long)h * w;
  SR_CHECK_ARG(hw < (1ll << 26), "sr_tof_align_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(sr::aligned16(flows) && sr::aligned16(out), "sr_tof_align_f32: CB8 tensors must be 16-byte aligned");
  SR_CHECK_ARG(flow_img_stride % 4 == 0 && out_img_stride % 4 == 0, "sr_tof_align_f32: image strides must be multiples of 4 floats");
  SR_CHECK_ARG(flow_img_stride >= hw * 8 && out_img_stride >= hw * 24, "sr_tof_align_f32: an image stride is smaller than the image");
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 191, 21, 24, b, h, w, 8.0 * 18.0 * b * hw, 4.0 * b * hw * (3.0 + 6.0 * 14.0 + 24.0));
  hipLaunchKernelGGL(tof_align_kernel, dim3((unsigned)((hw + 255) / 256), 1, (unsigned)b), dim3(256), 0, stream, clip, flows,
                     flow_img_stride, out, out_img_stride, ref_idx, h, w);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_tof_align_f32 launch");
  return SR_OK;
}

extern "C" int sr_tof_finish_f32(const float* y, long long y_img_stride, const float* lr_ref, long long lr_img_stride, float* out, int n,
                                 int h, int w, const float* mean3, const float* std3, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(y && lr_ref && out && mean3 && std3, "sr_tof_finish_f32: null y / lr_ref / out / mean3 / std3");
  SR_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0, "sr_tof_finish_f32: bad shape n=%d h=%d w=%d", n, h, w);
  const long long hw = (long long)h * w;
  SR_CHECK_ARG(hw < (1ll << 28), "sr_tof_finish_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(sr::aligned16(y) && y_img_stride % 4 == 0, "sr_tof_finish_f32: y must be 16-byte aligned with an image stride that is a multiple of 4 floats");
  SR_CHECK_ARG(y_img_stride >= hw * 8 && lr_img_stride >= hw * 3, "sr_tof_finish_f32: an image stride is smaller than the image");
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = mean3[c];
    nm.stdv[c] = std3[c];
  }
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 192, 3, 3, n, h, w, 9.0 * n * hw, 4.0 * n * hw * (8.0 + 3.0 + 3.0));
  hipLaunchKernelGGL(tof_finish_kernel, dim3((unsigned)((hw + 255) / 256), 1, (unsigned)n), dim3(256), 0, stream, y, y_img_stride, lr_ref,
                     lr_img_stride, out, (int)hw, nm);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_tof_finish_f32 launch");
  return SR_OK;
}
