// What EDVR's bf16 inference forward needs on CB16 tensors besides the 3x3 and the deformable conv (include/sr_hip_edvr_bf16.h):
// a 1x1 conv on v_mfma_f32_32x32x16_bf16, the even-position subsample behind a stride-1 conv, TSA's two poolings in one pass,
// its temporal correlation and its gate.  Forward only; fp32 arithmetic, one rounding to bf16 per stored value.
//
// The 1x1 conv is D[cout][pixel] += W[cout][k] X[k][pixel] with no spatial structure, so the pixels of an image are one flat
// index: a wave owns 64 consecutive pixels (two MFMA pixel tiles), a workgroup of 4 waves 256.  The B operand of lane (pixel j,
// half h) is the 16 bytes of channels 8h..8h+7 of its pixel, loaded straight from memory: a wave instruction reads 32 whole
// 32-byte pixels = 1 KiB contiguous, and nothing is shared between waves, so X never passes through LDS.  The weights of the cout
// group (32 * COT couts x cin) are what every wave re-reads: they are staged once per workgroup by LDS-DMA, [cin / 16][32 * COT][32 B]
// with conv_bf16.hip's half-swap swizzle, at most 32 blocks (512 channels, 32 * COT KiB) per pass.  Memory bound: 768 B per pixel
// at 320 -> 64 against 2 * 320 * 64 FLOP.
#include <algorithm>

#include "cb16_tile.h"
#include "../../include/sr_hip_edvr_bf16.h"

using namespace cb16;

namespace {

constexpr int PW_PASS = 32;  // channel blocks of weights resident in LDS at a time

struct PwParams {
  const char* x;
  const char* w;
  const float* bias;
  char* out;
  long long x_nb, out_nb;  // image strides in bytes
  long long HW;
  int cin_blocks, cout_blocks;
  int tiles;  // 256-pixel tiles per image
  float slope;
};

template <int COT>
__global__ __launch_bounds__(256) void pw16_conv_kernel(const PwParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int PT = 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int n = blockIdx.x / p.tiles, tile = blockIdx.x - n * p.tiles;
  const int cog = blockIdx.y;
  const char* wg = p.w + (size_t)cog * p.cin_blocks * (COT * 1024);
  const __amdgpu_buffer_rsrc_t w_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)wg, 0, (unsigned)((long long)p.cin_blocks * COT * 1024), 0x00020000);
  const unsigned wvo = (lane ^ ((lane >> 4) & 1)) * 16;  // unit (cout i, half) <- half ^ bit3(i)
  const int wlane = j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  long long pix[PT];
  const char* xp[PT];
#pragma unroll
  for (int r = 0; r < PT; ++r) {
    const long long q = (long long)tile * 256 + (wave * PT + r) * 32 + j;
    pix[r] = q < p.HW ? q : -1ll;
    xp[r] = p.x + (long long)n * p.x_nb + (q < p.HW ? q : 0) * 32 + h * 16;
  }

  f32x16 acc[COT][PT];
#pragma unroll
  for (int a = 0; a < COT; ++a)
#pragma unroll
    for (int b = 0; b < PT; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const long long plane_b = p.HW * 32;
  for (int c0 = 0; c0 < p.cin_blocks; c0 += PW_PASS) {
    const int nb = min(PW_PASS, p.cin_blocks - c0);
    if (c0) __syncthreads();  // every wave has read the previous pass's weights
    for (int u = wave; u < nb * COT; u += 4) sr::blds16(w_rs, wvo, (unsigned)(c0 * COT + u) * 1024u, smem + u * 1024);
    __syncthreads();
    for (int cb = 0; cb < nb; ++cb) {
      bf16x8 b[PT], a[COT];
#pragma unroll
      for (int r = 0; r < PT; ++r) {
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        b[r] = pix[r] >= 0 ? *(const bf16x8*)(xp[r] + (long long)(c0 + cb) * plane_b) : z;
      }
#pragma unroll
      for (int c = 0; c < COT; ++c) a[c] = *(const bf16x8*)(smem + (cb * COT + c) * 1024 + wlane);
#pragma unroll
      for (int c = 0; c < COT; ++c)
#pragma unroll
        for (int r = 0; r < PT; ++r) acc[c][r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[c], b[r], acc[c][r], 0, 0, 0);
    }
  }
  epilogue<COT, PT>(acc, p.bias, p.slope, p.out + (long long)n * p.out_nb, p.HW, pix, cog, p.cout_blocks, h);
}

// OIHW fp32 [cout][cin] -> wp[co / gc][ci >> 4][co % gc][ci & 15]; one thread per weight (the image is zeroed first)
__global__ void pw16_pack_kernel(const float* __restrict__ w, int cout, int cin, __bf16* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cout * cin) return;
  const int ci = i % cin, co = i / cin;
  const int gc = sr::group_couts(cout), cbs = cin / 16;
  wp[(((long long)(co / gc) * cbs + (ci >> 4)) * gc + co % gc) * 16 + (ci & 15)] = (__bf16)w[i];
}

__global__ void pw16_pack_bias_kernel(const float* __restrict__ b, int cout, int cp, float* __restrict__ bp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cp) bp[i] = (b && i < cout) ? b[i] : 0.f;
}

// ------------------------------------------------------------------------------------------------ memory-bound kernels
// One 16-byte half pixel (8 channels) of a CB16 window [n][cb][h][w][16] per thread: i = ((n * cb + blk) * h * w + pix) * 2 + half.
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

__global__ __launch_bounds__(256) void cb16_subsample2_kernel(const __bf16* __restrict__ x, long long x_ns, __bf16* __restrict__ out,
                                                              long long out_ns, int cb, int h, int w, int ho, int wo,
                                                              long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const HalfPix q = half_pix(i, cb, (long long)ho * wo);
  const int oy = (int)(q.pix / wo), ox = (int)(q.pix - (long long)oy * wo);
  const u32x4 v = *(const u32x4*)(x + q.n * x_ns + (((long long)q.blk * h + 2 * oy) * w + 2 * ox) * 16 + q.half * 8);
  *(u32x4*)(out + q.n * out_ns + ((long long)q.blk * ho * wo + q.pix) * 16 + q.half * 8) = v;
}

// one output half pixel per thread; taps in row-major order, pad skipped (max) / counted as 0 (sum)
__global__ __launch_bounds__(256) void pool16_s2_fwd_kernel(const __bf16* __restrict__ x, long long x_ns, __bf16* __restrict__ omax,
                                                            long long max_ns, __bf16* __restrict__ oavg, long long avg_ns, int cb,
                                                            int h, int w, int ho, int wo, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const HalfPix q = half_pix(i, cb, (long long)ho * wo);
  const int oy = (int)(q.pix / wo), ox = (int)(q.pix - (long long)oy * wo);
  const __bf16* xp = x + q.n * x_ns + (long long)q.blk * h * w * 16 + q.half * 8;
  const float ninf = -__builtin_inff();
  float m[8], s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = ninf, s[e] = 0.f;
#pragma unroll
  for (int ty = 0; ty < 3; ++ty) {
    const int yy = 2 * oy - 1 + ty;
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
      const int xx = 2 * ox - 1 + tx;
      if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
      const u32x4 v = *(const u32x4*)(xp + ((long long)yy * w + xx) * 16);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf_at(v, e);
        m[e] = f > m[e] ? f : m[e];
        s[e] += f;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = s[e] / 9.f;
  const long long o = ((long long)q.blk * ho * wo + q.pix) * 16 + q.half * 8;
  *(u32x4*)(omax + q.n * max_ns + o) = pack8(m);  // a maximum of bf16 values is a bf16 value: the conversion is exact
  *(u32x4*)(oavg + q.n * avg_ns + o) = pack8(s);
}

// one (frame, pixel) per thread
__global__ __launch_bounds__(256) void tsa16_corr_kernel(const __bf16* __restrict__ emb, long long emb_ns, const __bf16* __restrict__ ref,
                                                         long long ref_ns, const __bf16* __restrict__ al, long long al_ns,
                                                         float* __restrict__ prob, __bf16* __restrict__ out, long long out_ns, int t,
                                                         int cb, long long hw, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long pix = i % hw, bt = i / hw, b = bt / t;
  const __bf16* ep = emb + bt * emb_ns + pix * 16;
  const __bf16* rp = ref + b * ref_ns + pix * 16;
  float s = 0.f;
  for (int k = 0; k < cb; ++k) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const u32x4 a = *(const u32x4*)(ep + k * hw * 16 + half * 8), r = *(const u32x4*)(rp + k * hw * 16 + half * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += bf_at(a, e) * bf_at(r, e);
    }
  }
  const float pr = sigmoidf_(s);
  if (prob) prob[i] = pr;
  const __bf16* ap = al + bt * al_ns + pix * 16;
  __bf16* op = out + bt * out_ns + pix * 16;
  for (int k = 0; k < cb; ++k) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const u32x4 a = *(const u32x4*)(ap + k * hw * 16 + half * 8);
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = bf_at(a, e) * pr;
      *(u32x4*)(op + k * hw * 16 + half * 8) = pack8(v);
    }
  }
}

__global__ __launch_bounds__(256) void tsa16_gate_kernel(const __bf16* __restrict__ feat, long long feat_ns, const __bf16* __restrict__ attn,
                                                         long long attn_ns, const __bf16* __restrict__ add, long long add_ns,
                                                         __bf16* __restrict__ out, long long out_ns, long long per_img,
                                                         long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long n = i / per_img, o = (i - n * per_img) * 8;
  const u32x4 f = *(const u32x4*)(feat + n * feat_ns + o), a = *(const u32x4*)(attn + n * attn_ns + o);
  const u32x4 ad = *(const u32x4*)(add + n * add_ns + o);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (bf_at(f, e) * sigmoidf_(bf_at(a, e))) * 2.f + bf_at(ad, e);
  *(u32x4*)(out + n * out_ns + o) = pack8(v);
}

bool strides_ok(long long need, std::initializer_list<long long> strides) {
  for (long long s : strides)
    if (s % 8 || s < need) return false;
  return true;
}

bool grid_ok(long long total) { return total > 0 && (total + 255) / 256 < (1ll << 31); }

template <int COT>
int pw_launch(const PwParams& p, int n, int groups, int cin, int cout, int h, int w, hipStream_t stream) {
  const int lds = std::min(p.cin_blocks, PW_PASS) * COT * 1024;
  auto kern = pw16_conv_kernel<COT>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, PW_PASS * COT * 1024)) return rc;
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)n * h * w;
    sr::prof_rec(stream, 125, cin, cout, n, h, w, 2.0 * cin * cout * px, 2.0 * px * (cin + cout));
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles * n), groups), dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("conv1x1_bf16 launch");
  return SR_OK;
}

}  // namespace

#define EDVR16_GRID(total) dim3((unsigned)(((total) + 255) / 256)), dim3(256), 0, stream

extern "C" size_t sr_conv1x1_packed_weight_elems_bf16(int cout, int cin) {
  if (cout <= 0 || cin <= 0 || cin % 16) return 0;
  return (size_t)((cout + 31) / 32 * 32) * cin;
}

extern "C" int sr_conv1x1_pack_bf16(const float* weight, const float* bias, int cout, int cin, void* wpacked, float* bpacked,
                                    void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(weight && wpacked && cout > 0 && cin > 0, "sr_conv1x1_pack_bf16: bad argument");
  SR_CHECK_ARG(cin % 16 == 0, "sr_conv1x1_pack_bf16: cin=%d must be a multiple of 16 (CB16)", cin);
  SR_CHECK_ARG((long long)cout * cin < (1ll << 31), "sr_conv1x1_pack_bf16: weight too large");
  if (hipMemsetAsync(wpacked, 0, sr_conv1x1_packed_weight_elems_bf16(cout, cin) * 2, stream) != hipSuccess) {
    sr::set_error("sr_conv1x1_pack_bf16: memset failed");
    return SR_ELAUNCH;
  }
  const int total = cout * cin;
  hipLaunchKernelGGL(pw16_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, weight, cout, cin, (__bf16*)wpacked);
  SR_CHECK_LAUNCH("conv1x1 pack");
  if (bpacked) {
    const int cp = (cout + 31) / 32 * 32;
    hipLaunchKernelGGL(pw16_pack_bias_kernel, dim3((cp + 255) / 256), dim3(256), 0, stream, bias, cout, cp, bpacked);
    SR_CHECK_LAUNCH("conv1x1 bias pack");
  }
  return SR_OK;
}

extern "C" int sr_conv1x1_bf16(const void* x, int64_t x_ns, const void* wpacked, const float* bpacked, void* out, int64_t out_ns, int n,
                               int cin, int cout, int h, int w, float act_slope, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && wpacked && out, "sr_conv1x1_bf16: null x / wpacked / out");
  SR_CHECK_ARG(n > 0 && cin > 0 && cout > 0 && h > 0 && w > 0, "sr_conv1x1_bf16: bad shape");
  SR_CHECK_ARG(cin % 16 == 0, "sr_conv1x1_bf16: cin=%d must be a multiple of 16 (CB16)", cin);
  SR_CHECK_ARG(aligned16({x, wpacked, bpacked, out}), "sr_conv1x1_bf16: pointers must be 16-byte aligned");
  const long long hw = (long long)h * w, cob = (cout + 15) / 16;
  SR_CHECK_ARG(strides_ok(hw * cin, {x_ns}) && strides_ok(hw * 16 * cob, {out_ns}),
               "sr_conv1x1_bf16: an image stride is smaller than the image or not a multiple of 8");
  SR_CHECK_ARG((long long)cin * 128 < (1ll << 31), "sr_conv1x1_bf16: cin too large for the weight descriptor");
  PwParams p = {};
  p.x = (const char*)x;
  p.w = (const char*)wpacked;
  p.bias = bpacked;
  p.out = (char*)out;
  p.x_nb = x_ns * 2;
  p.out_nb = out_ns * 2;
  p.HW = hw;
  p.cin_blocks = cin / 16;
  p.cout_blocks = (int)cob;
  p.slope = act_slope;
  const long long tiles = (hw + 255) / 256;
  SR_CHECK_ARG(tiles * n < (1ll << 31), "sr_conv1x1_bf16: grid too large");
  p.tiles = (int)tiles;
  const int gc = sr::group_couts(cout);
  const int groups = ((cout + 31) / 32 * 32) / gc;
  SR_CHECK_ARG(groups < 65536, "sr_conv1x1_bf16: cout too large");
  return gc == 64 ? pw_launch<2>(p, n, groups, cin, cout, h, w, stream) : pw_launch<1>(p, n, groups, cin, cout, h, w, stream);
}

extern "C" int sr_cb16_subsample2_bf16(const void* x, int64_t x_ns, void* out, int64_t out_ns, int n, int cb, int h, int w,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && out && n > 0 && cb > 0 && h > 0 && w > 0, "sr_cb16_subsample2_bf16: bad argument");
  SR_CHECK_ARG(aligned16({x, out}), "sr_cb16_subsample2_bf16: pointers must be 16-byte aligned");
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  SR_CHECK_ARG(strides_ok((long long)cb * h * w * 16, {x_ns}) && strides_ok((long long)cb * ho * wo * 16, {out_ns}),
               "sr_cb16_subsample2_bf16: an image stride is smaller than the image or not a multiple of 8");
  const long long total = (long long)n * cb * ho * wo * 2;
  SR_CHECK_ARG(grid_ok(total), "sr_cb16_subsample2_bf16: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 126, cb * 16, cb * 16, n, h, w, 0.0, 4.0 * total * 8);
  hipLaunchKernelGGL(cb16_subsample2_kernel, EDVR16_GRID(total), (const __bf16*)x, (long long)x_ns, (__bf16*)out, (long long)out_ns, cb,
                     h, w, ho, wo, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("cb16_subsample2 launch");
  return SR_OK;
}

extern "C" int sr_pool3x3s2_fwd_bf16(const void* x, int64_t x_ns, void* out_max, int64_t max_ns, void* out_avg, int64_t avg_ns, int n,
                                     int cb, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && out_max && out_avg && n > 0 && cb > 0 && h > 0 && w > 0, "sr_pool3x3s2_fwd_bf16: bad argument");
  SR_CHECK_ARG(aligned16({x, out_max, out_avg}), "sr_pool3x3s2_fwd_bf16: pointers must be 16-byte aligned");
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  SR_CHECK_ARG(strides_ok((long long)cb * h * w * 16, {x_ns}) && strides_ok((long long)cb * ho * wo * 16, {max_ns, avg_ns}),
               "sr_pool3x3s2_fwd_bf16: an image stride is smaller than the image or not a multiple of 8");
  const long long total = (long long)n * cb * ho * wo * 2;
  SR_CHECK_ARG(grid_ok(total), "sr_pool3x3s2_fwd_bf16: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 127, cb * 16, cb * 32, n, h, w, 17.0 * n * cb * 16 * ho * wo, 2.0 * n * cb * 16 * ((double)h * w + 2.0 * ho * wo));
  hipLaunchKernelGGL(pool16_s2_fwd_kernel, EDVR16_GRID(total), (const __bf16*)x, (long long)x_ns, (__bf16*)out_max, (long long)max_ns,
                     (__bf16*)out_avg, (long long)avg_ns, cb, h, w, ho, wo, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("pool3x3s2_fwd_bf16 launch");
  return SR_OK;
}

extern "C" int sr_tsa_corr_fwd_bf16(const void* emb, int64_t emb_ns, const void* emb_ref, int64_t ref_ns, const void* aligned,
                                    int64_t al_ns, float* prob, void* out, int64_t out_ns, int b, int t, int c, int h, int w,
                                    void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(emb && emb_ref && aligned && out, "sr_tsa_corr_fwd_bf16: null pointer");
  SR_CHECK_ARG(b > 0 && t > 0 && c > 0 && c % 16 == 0 && h > 0 && w > 0, "sr_tsa_corr_fwd_bf16: bad shape (c=%d must be a multiple of 16)", c);
  SR_CHECK_ARG(aligned16({emb, emb_ref, aligned, out}) && (uintptr_t)prob % 4 == 0, "sr_tsa_corr_fwd_bf16: pointers must be 16-byte aligned");
  const long long hw = (long long)h * w, total = (long long)b * t * hw;
  SR_CHECK_ARG(strides_ok(hw * c, {emb_ns, ref_ns, al_ns, out_ns}),
               "sr_tsa_corr_fwd_bf16: an image stride is smaller than the image or not a multiple of 8");
  SR_CHECK_ARG(grid_ok(total), "sr_tsa_corr_fwd_bf16: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 128, c, c, b * t, h, w, 3.0 * total * c, 2.0 * total * 3.0 * c + 2.0 * b * hw * c + (prob ? 4.0 * total : 0.0));
  hipLaunchKernelGGL(tsa16_corr_kernel, EDVR16_GRID(total), (const __bf16*)emb, (long long)emb_ns, (const __bf16*)emb_ref,
                     (long long)ref_ns, (const __bf16*)aligned, (long long)al_ns, prob, (__bf16*)out, (long long)out_ns, t, c / 16, hw,
                     total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("tsa_corr_fwd_bf16 launch");
  return SR_OK;
}

extern "C" int sr_tsa_gate_fwd_bf16(const void* feat, int64_t feat_ns, const void* attn, int64_t attn_ns, const void* attn_add,
                                    int64_t add_ns, void* out, int64_t out_ns, int n, int cb, int h, int w, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(feat && attn && attn_add && out && n > 0 && cb > 0 && h > 0 && w > 0, "sr_tsa_gate_fwd_bf16: bad argument");
  SR_CHECK_ARG(aligned16({feat, attn, attn_add, out}), "sr_tsa_gate_fwd_bf16: pointers must be 16-byte aligned");
  const long long per_img = (long long)cb * h * w * 2, total = per_img * n;
  SR_CHECK_ARG(strides_ok(per_img * 8, {feat_ns, attn_ns, add_ns, out_ns}),
               "sr_tsa_gate_fwd_bf16: an image stride is smaller than the image or not a multiple of 8");
  SR_CHECK_ARG(grid_ok(total), "sr_tsa_gate_fwd_bf16: grid too large");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 129, cb * 16, cb * 16, n, h, w, 8.0 * total * 8, 2.0 * total * 8 * 4);
  hipLaunchKernelGGL(tsa16_gate_kernel, EDVR16_GRID(total), (const __bf16*)feat, (long long)feat_ns, (const __bf16*)attn,
                     (long long)attn_ns, (const __bf16*)attn_add, (long long)add_ns, (__bf16*)out, (long long)out_ns, per_img, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("tsa_gate_fwd_bf16 launch");
  return SR_OK;
}
