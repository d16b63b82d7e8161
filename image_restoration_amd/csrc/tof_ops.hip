// The pieces of TOFlow on gfx950 (include/sr_hip_tof.h): the 9x9 convolution of the reconstruction module, SPyNetTOF's level
// input, the aligned 7-frame stack and the finish.
//
// Reference: TOFlow (basicsr/archs/tof_arch.py) estimates six flows with SPyNetTOF (four pyramid levels of five 7x7 convs with
// BatchNorm), warps the six neighbours onto the reference frame, and runs conv 9x9 (21 -> 64), conv 9x9 (64 -> 64), two 1x1 convs
// and a residual.  The 7x7 convs run on flow_ops.hip with the BatchNorm folded on the host; the 1x1 convs on ridnet_ops.hip.
//
// 9x9 convolution: conv_body<2, 2> of flow_device.h, the implicit GEMM described at the head of flow_ops.hip, with KS = 9 taken
// from C9Params.  Output tile = 8 rows x 32 columns x 64 couts; wave w owns rows 2w, 2w + 1.  K = 81 * cin_pad is walked in chunks
// of (one 8-channel block, one tap row): the halo'd X tile [8 + 8][40][8] (20 KiB) is staged once per channel block, the weights
// [9 taps][64][8] (18 KiB) once per chunk, double buffered: 2 * (20 + 18) KiB = 76 KiB, so two workgroups share a CU's 160 KiB.
// Per chunk and wave: 9 * 4 ds_read_b128 feed 144 MFMAs of 64 cycles.  What C9Params lacks is compiled out of the body: cout groups
// over blockIdx.y, the cout_blocks test and res1.  What it adds is compiled in: the source of conv_1 has 21 channels in 3 blocks,
// and in the last block the lanes that hold channels 21-23 replace what they read by zero (three selects per B operand), so those
// channels may hold anything.
#include <math.h>

#include "../../include/sr_hip_tof.h"
#include "flow_device.h"
#include "sr_internal.h"

using namespace flowdev;  // the conv body, the level-input body and the warp rule, shared with flow_ops.hip

namespace {

// ------------------------------------------------------------------------------------------------------------ conv 9x9
// conv_body<2, 2> of flow_device.h on C9Params: 64 couts, 2 rows per wave, 8 rows per tile
__global__ __launch_bounds__(256, 2) void tof_conv9x9_f32_kernel(const C9Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  conv_body<2, 2, false>(p, smem);
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
// level_input_body of flow_device.h with zeros padding: image n is pair n % group of clip n / group; the frame that is warped
// steps over the reference (frame ``skip``)
__global__ __launch_bounds__(256) void tof_level_input_kernel(const float* __restrict__ ref, long long ref_gs,
                                                              const float* __restrict__ supp, long long supp_gs, int group, int skip,
                                                              const float* __restrict__ flow_prev, float* __restrict__ out,
                                                              float* __restrict__ up_out, int H, int W) {
  const int n = blockIdx.z, g = n / group, kk = n - g * group;
  level_input_body<0>(ref + (long long)g * ref_gs, supp + (long long)g * supp_gs + (long long)(kk + (kk >= skip ? 1 : 0)) * 3 * (H * W),
                      flow_prev, out, up_out, H, W);  // zeros padding
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
  if (prof) sr::prof_rec(stream, 189, cin, cout, 1, 9, 9, 0.0, 4.0 * (total + 81.0 * cin * cout));
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
  p.tiles_y = sr::cdiv(d->h, conv_tile_rows<2>());
  SR_CHECK_ARG((long long)p.tiles_x * p.tiles_y * d->n < (1ll << 31), "sr_tof_conv9x9_f32: grid too large");
  constexpr int lds = conv_lds_bytes<2, 2, C9Params::KS>();
  static_assert(lds == 77824, "two workgroups of the 9x9 kernel share a CU's 160 KiB of LDS");
  if (int rc = sr::ensure_dynamic_lds((const void*)tof_conv9x9_f32_kernel, lds)) return rc;
  const dim3 grid((unsigned)(p.tiles_x * p.tiles_y * d->n), 1);
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * (double)hw;
    sr::prof_rec(stream, 188, d->cin, d->cout, d->n, d->h, d->w, 2.0 * 81.0 * d->cin * d->cout * px, 4.0 * px * (cinb * 8.0 + d->cout));
  }
  hipLaunchKernelGGL(tof_conv9x9_f32_kernel, grid, dim3(256), lds, stream, p);
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
  if (prof) sr::prof_rec(stream, 190, 8, 8, N, H, W, 40.0 * N * H * W, 4.0 * N * H * W * (3.0 + 12.0 + 2.0 + 16.0));
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
  if (prof) sr::prof_rec(stream, 191, 21, 24, b, h, w, 8.0 * 18.0 * b * hw, 4.0 * b * hw * (3.0 + 6.0 * 14.0 + 24.0));
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
  if (prof) sr::prof_rec(stream, 192, 3, 3, n, h, w, 9.0 * n * hw, 4.0 * n * hw * (8.0 + 3.0 + 3.0));
  hipLaunchKernelGGL(tof_finish_kernel, dim3((unsigned)((hw + 255) / 256), 1, (unsigned)n), dim3(256), 0, stream, y, y_img_stride, lr_ref,
                     lr_img_stride, out, (int)hw, nm);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_tof_finish_f32 launch");
  return SR_OK;
}
