// The sampling position of the fp32 modulated deformable convolution, once: the forward, the column kernel and the backward of
// dcn_ops.hip and the deterministic input gradient of dcn_det_ops.hip all sample where these functions say, so the position of the
// deterministic scatter is the forward's bit for bit by construction.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace dcndev {

// One sampling position (dmcn_im2col_bilinear and the `inside` test of its caller, deform_conv_cuda_kernel.cu:466-497, 618):
// the top-left corner, the four weights and which corners lie in the image.  Outside, no corner is valid.
// (dcn_ops_bf16.hip's tap_at keeps its own representation — a byte offset, validity bits, the mask folded into the weights — which
// its kernel was tuned around.)
struct Bilinear {
  int hl, wl;
  float lh, lw, hh, hw;
  bool v1, v2, v3, v4;
};

__device__ __forceinline__ Bilinear bilinear_at(float h_im, float w_im, int H, int W) {
  Bilinear b;
  const bool inside = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  if (!inside) h_im = w_im = 0.f;  // also NaN and huge offsets: nothing below is used
  const float fh = floorf(h_im), fw = floorf(w_im);
  b.hl = (int)fh;
  b.wl = (int)fw;
  b.lh = h_im - fh;
  b.lw = w_im - fw;
  b.hh = 1.f - b.lh;
  b.hw = 1.f - b.lw;
  const bool t = b.hl >= 0, bo = b.hl + 1 <= H - 1, l = b.wl >= 0, r = b.wl + 1 <= W - 1;
  b.v1 = inside && t && l;
  b.v2 = inside && t && r;
  b.v3 = inside && bo && l;
  b.v4 = inside && bo && r;
  return b;
}

__device__ __forceinline__ float channel_at(const float* t, long long HW, long long pix, int c) {
  return t[((long long)(c >> 3) * HW + pix) * 8 + (c & 7)];
}

__device__ __forceinline__ float mask_value(float m, int logit) { return logit ? 1.f / (1.f + expf(-m)) : m; }

// Where tap `tap` of the 3x3 kernel samples for the output pixel (y, x), given its two offsets
__device__ __forceinline__ Bilinear tap_position(int y, int x, int tap, float oh, float ow, int H, int W) {
  const int ti = tap / 3, tj = tap - 3 * ti;
  return bilinear_at((float)(y - 1 + ti) + oh, (float)(x - 1 + tj) + ow, H, W);
}

}  // namespace dcndev
