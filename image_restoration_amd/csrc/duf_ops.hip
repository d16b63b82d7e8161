// The pieces of DUF on gfx950 (include/sr_hip_duf.h): the (kt, 3, 3) and 1x1x1 convolutions over frame-major CB8 clips with
// an optional BatchNorm -> ReLU prologue on the operand, and the softmax + dynamic 5x5 filter + residual + pixel-shuffle tail.
//
// Reference: DUF (basicsr/archs/duf_arch.py) runs conv3d (1,3,3), dense blocks of [BN, ReLU, conv 1x1x1, BN, ReLU, conv (3,3,3)]
// whose outputs are concatenated, three such blocks without temporal padding (7 -> 1 frames), BN, ReLU, conv (1,3,3) to 256, two
// pairs of 1x1x1 head convs, and a per-pixel 5x5 filter on the centre frame.
//
// Convolution: an implicit GEMM D[cout][pixel] += W[cout][k] * X[k][pixel], k = (cin, frame tap, tap), on
// v_mfma_f32_16x16x4_f32: A = weights (lane l: cout l & 15, k l >> 4), B = activations (pixel l & 15, k l >> 4), D: lane l holds
// couts 4 * (l >> 4) .. + 3 of pixel l & 15, so a lane's accumulator is one 16-byte store into CB8.  Lane group q = l >> 4 reads
// channels (2q, 2q + 1) of its pixel as 8 bytes and feeds two MFMAs: channels (0, 2, 4, 6), then (1, 3, 5, 7).  Workgroup = 4
// waves, output tile = 8 rows x 32 columns x 16 * CT couts of one frame; wave w owns rows 2w, 2w + 1 (four 16-pixel groups).
// K is walked in chunks of (one 8-channel block, one frame tap).  A chunk's halo'd tile and weights are loaded into registers
// while the previous chunk is computed, transformed (prologue, padding and pad-channel masks) and written to the other LDS
// buffer after it: one barrier per chunk.  The LDS images are plain [pixel][8] and [tap][cout][8]: the 64 lanes of a
// ds_read_b64 cover 512 contiguous bytes.
#include <math.h>

#include "../../include/sr_hip_duf.h"
#include "sr_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kTH = 8, kTW = 32;  // output tile

struct DParams {
  const float* in;
  const float* w;
  const float* bias;
  const float* scale;
  const float* shift;
  float* out;
  long long in_fs, in_cs, out_fs, out_cs;
  int cin, cinb, cout_blocks, kt, pad_t, T, Tout, H, W, tiles_x, tiles_y, relu, out_cb0;
};

template <int KS, int CT>
struct Geo {
  static constexpr int P = KS / 2, ROWW = kTW + KS - 1, ROWS = kTH + KS - 1;
  static constexpr int XPIX = ROWS * ROWW, NXP = XPIX * 2, NXR = (NXP + 255) / 256;      // 16-byte pieces of the tile
  static constexpr int XBYTES = (XPIX * 32 + 15) / 16 * 16;
  static constexpr int WFLOATS = KS * KS * 16 * CT * 8, NWP = WFLOATS / 4, NWR = (NWP + 255) / 256;
  static constexpr int WBYTES = WFLOATS * 4;
  static constexpr int LDS = 2 * (XBYTES + WBYTES);
};

template <int KS, int CT>
__device__ __forceinline__ void duf_conv_body(const DParams& p, char* smem) {
  using G = Geo<KS, CT>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, q4 = lane >> 4;
  int t = blockIdx.x;
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int img = t / p.tiles_y;            // clip * Tout + output frame
  const int clip = img / p.Tout, to = img - clip * p.Tout;
  const int g = blockIdx.y;                 // cout group of 16 * CT
  const int x0 = tx * kTW, y0 = ty * kTH;
  const int HW = p.H * p.W;

  // frame taps inside the clip: source frame = to + dt - pad_t (kt = 1: to)
  const int dt0 = p.pad_t - to > 0 ? p.pad_t - to : 0;
  const int dt1 = p.T + p.pad_t - to < p.kt ? p.T + p.pad_t - to : p.kt;
  const int ndt = dt1 - dt0;
  const int nchunk = ndt > 0 ? p.cinb * ndt : 0;
  const float* in_clip = p.in + (long long)clip * p.in_cs;
  const float* w_g = p.w + (long long)g * p.cinb * p.kt * G::WFLOATS;

  // this thread's pieces of the halo'd tile: float offset inside a frame's channel block, -1 outside the image
  const int half = tid & 1;
  int xoff[G::NXR];
#pragma unroll
  for (int r = 0; r < G::NXR; ++r) {
    const int q = r * 256 + tid;
    const int pix = q >> 1;
    const int row = pix / G::ROWW, col = pix - row * G::ROWW;
    const int gy = y0 - G::P + row, gx = x0 - G::P + col;
    const bool valid = pix < G::XPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
    xoff[r] = valid ? (gy * p.W + gx) * 8 + half * 4 : -1;
  }

  char* const xs0 = smem;
  char* const ws0 = smem + 2 * G::XBYTES;
  f32x4 xr[G::NXR], wr[G::NWR], sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  int lim = 4;  // how many of this piece's 4 channels are real

  auto prefetch = [&](int c) {
    const int cb = c / ndt, dt = dt0 + (c - cb * ndt);
    const float* frame = in_clip + (long long)(to + dt - p.pad_t) * p.in_fs + (long long)cb * HW * 8;
#pragma unroll
    for (int r = 0; r < G::NXR; ++r) {
      xr[r] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (xoff[r] >= 0) xr[r] = *(const f32x4*)(frame + xoff[r]);
    }
    const float* wc = w_g + (long long)(cb * p.kt + dt) * G::WFLOATS;
#pragma unroll
    for (int r = 0; r < G::NWR; ++r) {
      const int q = r * 256 + tid;
      if (q < G::NWP) wr[r] = *(const f32x4*)(wc + q * 4);
    }
    lim = p.cin - cb * 8 - half * 4;
    if (p.scale) {
      const int c0 = cb * 8 + half * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sc[e] = c0 + e < p.cin ? p.scale[c0 + e] : 1.f;
        sh[e] = c0 + e < p.cin ? p.shift[c0 + e] : 0.f;
      }
    }
  };
  auto store = [&](int buf) {
    char* xs = xs0 + buf * G::XBYTES;
    char* ws = ws0 + buf * G::WBYTES;
#pragma unroll
    for (int r = 0; r < G::NXR; ++r) {
      const int q = r * 256 + tid;
      if (q >= G::NXP) continue;
      f32x4 v = xr[r];
      if (p.scale) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float a = v[e] * sc[e];
          a = a + sh[e];
          v[e] = a > 0.f ? a : 0.f;
        }
      }
      const bool valid = xoff[r] >= 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (valid && e < lim) ? v[e] : 0.f;   // padding and pad channels: after the prologue
      *(f32x4*)(xs + q * 16) = v;
    }
#pragma unroll
    for (int r = 0; r < G::NWR; ++r) {
      const int q = r * 256 + tid;
      if (q < G::NWP) *(f32x4*)(ws + q * 16) = wr[r];
    }
  };

  f32x4 acc[CT][4];
#pragma unroll
  for (int a = 0; a < CT; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int xlane = ((wave * 2) * G::ROWW + m) * 32 + q4 * 8;
  const int wlane = m * 32 + q4 * 8;
  auto compute = [&](int buf) {
    const char* xs = xs0 + buf * G::XBYTES + xlane;
    const char* ws = ws0 + buf * G::WBYTES + wlane;
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) {
#pragma unroll
      for (int dx = 0; dx < KS; ++dx) {
        f32x2 a[CT], b[4];
#pragma unroll
        for (int c = 0; c < CT; ++c) a[c] = *(const f32x2*)(ws + ((dy * KS + dx) * 16 * CT + c * 16) * 32);
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) b[pt] = *(const f32x2*)(xs + (((pt >> 1) + dy) * G::ROWW + (pt & 1) * 16 + dx) * 32);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int pt = 0; pt < 4; ++pt) acc[c][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][s], b[pt][s], acc[c][pt], 0, 0, 0);
      }
    }
  };

  if (nchunk > 0) {
    prefetch(0);
    store(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
      if (c + 1 < nchunk) prefetch(c + 1);
      compute(c & 1);
      if (c + 1 < nchunk) store((c + 1) & 1);  // that buffer was last read in chunk c - 1, before the barrier that ended it
      __syncthreads();
    }
  }

  // ---- epilogue: bias, ReLU
  float* out_img = p.out + (long long)clip * p.out_cs + (long long)to * p.out_fs;
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int y = y0 + wave * 2 + (pt >> 1), x = x0 + (pt & 1) * 16 + m;
    if (y >= p.H || x >= p.W) continue;
    const long long pixoff = (long long)y * p.W + x;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int co = (g * CT + c) * 16 + q4 * 4;   // first of this lane's 4 couts
      const int ob = co >> 3;
      if (ob >= p.cout_blocks) continue;
      f32x4 v = acc[c][pt] + *(const f32x4*)(p.bias + co);
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
      }
      *(f32x4*)(out_img + ((long long)(p.out_cb0 + ob) * HW + pixoff) * 8 + (co & 4)) = v;
    }
  }
}

template <int CT>
__global__ __launch_bounds__(256, 2) void duf_conv3d_f32_kernel(const DParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  duf_conv_body<3, CT>(p, smem);
}

__global__ __launch_bounds__(256, 2) void duf_pw_f32_kernel(const DParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  duf_conv_body<1, 4>(p, smem);
}

// Weight image [cout group][cin block][frame tap][tap][gc couts][8 channels], then the groups * gc biases.
__global__ __launch_bounds__(256) void duf_conv_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ out, int cout, int cin, int cinb, int kt, int taps,
                                                            int gc, long long wfloats, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  if (idx >= wfloats) {
    const int b = (int)(idx - wfloats);
    out[idx] = (bias && b < cout) ? bias[b] : 0.f;
    return;
  }
  const int ch = (int)(idx & 7);
  long long rest = idx >> 3;
  const int ci_g = (int)(rest % gc);
  rest /= gc;
  const int tap = (int)(rest % taps);
  rest /= taps;
  const int dt = (int)(rest % kt);
  rest /= kt;
  const int cb = (int)(rest % cinb), g = (int)(rest / cinb);
  const int co = g * gc + ci_g, ci = cb * 8 + ch;
  out[idx] = (co < cout && ci < cin) ? w[(((long long)co * cin + ci) * kt + dt) * taps + tap] : 0.f;
}

int conv3d_ct(int cout) { return cout == 16 ? 1 : cout == 32 ? 2 : (cout == 64 || cout == 256) ? 4 : 0; }
bool conv3d_served(int cout, int cin, int kt) {
  return conv3d_ct(cout) != 0 && (kt == 1 || kt == 3) && (cin == 3 || (cin >= 8 && cin <= 448 && cin % 8 == 0));
}
bool pw_served(int c) { return c >= 8 && c <= 432 && c % 8 == 0; }
// floats of the weight part of an image: groups * cinb * kt * taps * gc * 8
long long image_weight_floats(int cout, int cin, int kt, int taps, int gc) {
  return (long long)((cout + gc - 1) / gc) * ((cin + 7) / 8) * kt * taps * gc * 8;
}

int pack_common(const char* who, const float* weight, const float* bias, int cout, int cin, int kt, int taps, int gc, float* packed,
                hipStream_t stream) {
  SR_CHECK_ARG(weight && packed, "%s: null weight / packed", who);
  SR_CHECK_ARG(sr::aligned16(packed), "%s: packed must be 16-byte aligned", who);
  const long long wf = image_weight_floats(cout, cin, kt, taps, gc), total = wf + (long long)((cout + gc - 1) / gc) * gc;
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 195, cin, cout, 1, kt, taps, 0.0, 4.0 * (total + (double)taps * kt * cin * cout));
  hipLaunchKernelGGL(duf_conv_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, weight, bias, packed, cout, cin,
                     (cin + 7) / 8, kt, taps, gc, wf, total);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}

// The checks both convolutions share; fills p.  taps = 9 / 1, gc = couts per group.
int conv_common(const char* who, const sr_duf_conv_desc* d, int taps, int gc, DParams& p) {
  SR_CHECK_ARG(d->in && d->packed && d->out, "%s: null in / packed / out", who);
  SR_CHECK_ARG((d->scale == nullptr) == (d->shift == nullptr), "%s: scale and shift come together", who);
  SR_CHECK_ARG(d->b > 0 && d->t > 0 && d->h > 0 && d->w > 0, "%s: bad shape b=%d t=%d h=%d w=%d", who, d->b, d->t, d->h, d->w);
  const int tout = d->kt == 3 ? d->t - 2 * (1 - d->pad_t) : d->t;
  SR_CHECK_ARG(tout > 0, "%s: t=%d frames leave no output frame for kt=3 without temporal padding", who, d->t);
  SR_CHECK_ARG(sr::aligned16(d->in) && sr::aligned16(d->packed) && sr::aligned16(d->out), "%s: pointers must be 16-byte aligned", who);
  SR_CHECK_ARG(d->in_frame_stride % 4 == 0 && d->in_clip_stride % 4 == 0 && d->out_frame_stride % 4 == 0 && d->out_clip_stride % 4 == 0,
               "%s: strides must be multiples of 4 floats", who);
  SR_CHECK_ARG(d->relu == 0 || d->relu == 1, "%s: relu must be 0 or 1", who);
  SR_CHECK_ARG(d->out_cb0 >= 0 && d->out_cb0 <= 4096, "%s: out_cb0=%d is out of range", who, d->out_cb0);
  const long long hw = (long long)d->h * d->w;
  const int cinb = (d->cin + 7) / 8, coutb = d->cout / 8;
  const long long maxb = cinb > d->out_cb0 + coutb ? cinb : d->out_cb0 + coutb;
  SR_CHECK_ARG(hw < (1ll << 31) / (32 * maxb), "%s: frame too large for 32-bit plane offsets", who);
  SR_CHECK_ARG(d->in_frame_stride >= hw * 8 * cinb && d->out_frame_stride >= hw * 8 * (d->out_cb0 + coutb),
               "%s: a frame stride is smaller than the channel blocks used of a frame", who);
  SR_CHECK_ARG(d->in_clip_stride >= d->in_frame_stride * (d->t - 1) + hw * 8 * cinb &&
                   d->out_clip_stride >= d->out_frame_stride * (tout - 1) + hw * 8 * (d->out_cb0 + coutb),
               "%s: a clip stride is smaller than the frames of a clip", who);
  p.in = d->in;
  p.w = d->packed;
  p.bias = d->packed + image_weight_floats(d->cout, d->cin, d->kt, taps, gc);
  p.scale = d->scale;
  p.shift = d->shift;
  p.out = d->out;
  p.in_fs = d->in_frame_stride;
  p.in_cs = d->in_clip_stride;
  p.out_fs = d->out_frame_stride;
  p.out_cs = d->out_clip_stride;
  p.cin = d->cin;
  p.cinb = cinb;
  p.cout_blocks = coutb;
  p.kt = d->kt;
  p.pad_t = d->pad_t;
  p.T = d->t;
  p.Tout = tout;
  p.H = d->h;
  p.W = d->w;
  p.relu = d->relu;
  p.out_cb0 = d->out_cb0;
  p.tiles_x = sr::cdiv(d->w, kTW);
  p.tiles_y = sr::cdiv(d->h, kTH);
  SR_CHECK_ARG((long long)p.tiles_x * p.tiles_y * d->b * tout < (1ll << 31), "%s: grid too large", who);
  return SR_OK;
}

template <class K>
int launch_conv(const char* who, K kernel, int lds, const DParams& p, int id, const sr_duf_conv_desc* d, int taps, int groups,
                hipStream_t stream) {
  if (int rc = sr::ensure_dynamic_lds((const void*)kernel, lds)) return rc;
  const dim3 grid((unsigned)(p.tiles_x * p.tiles_y * d->b * p.Tout), (unsigned)groups);
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->b * p.Tout * d->h * d->w;
    sr::prof_rec(stream, id, d->cin, d->cout, d->b * p.Tout, d->h, d->w, 2.0 * taps * d->kt * d->cin * d->cout * px,
             4.0 * px * (p.cinb * 8.0 * d->kt * groups + d->cout));
  }
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}

// ------------------------------------------------------------------------------------------------------ dynamic filter
// grid (ceil(h * w * s * s / 256), 1, n): a thread computes the three colours of one (pixel, sub)
__global__ __launch_bounds__(256) void duf_filter_f32_kernel(const float* __restrict__ logits, long long l_ns, const float* __restrict__ res,
                                                             long long r_ns, const float* __restrict__ centre, long long c_ns,
                                                             float* __restrict__ out, int s, int H, int W, int softmax, int shuffle) {
  const int s2 = s * s, HW = H * W;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)HW * s2) return;
  const int n = blockIdx.z;
  const int pix = (int)(idx / s2), sub = (int)(idx - (long long)pix * s2);
  const int y = pix / W, x = pix - y * W;
  const float* L = logits + (long long)n * l_ns;
  float f[25];
#pragma unroll
  for (int tap = 0; tap < 25; ++tap) {
    const int ch = tap * s2 + sub;
    f[tap] = L[((long long)(ch >> 3) * HW + pix) * 8 + (ch & 7)];
  }
  if (softmax) {
    float mx = f[0];
#pragma unroll
    for (int tap = 1; tap < 25; ++tap) mx = f[tap] > mx ? f[tap] : mx;
    float sum = 0.f;
#pragma unroll
    for (int tap = 0; tap < 25; ++tap) {
      f[tap] = expf(f[tap] - mx);
      sum = sum + f[tap];
    }
#pragma unroll
    for (int tap = 0; tap < 25; ++tap) f[tap] = f[tap] / sum;
  }
  const float* cimg = centre + (long long)n * c_ns;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int tap = 0; tap < 25; ++tap) {
      const int yy = y + tap / 5 - 2, xx = x + tap % 5 - 2;
      const float v = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? cimg[(long long)c * HW + yy * W + xx] : 0.f;
      const float pr = f[tap] * v;
      acc = acc + pr;
    }
    const int ch = c * s2 + sub;
    if (res) acc = acc + res[(long long)n * r_ns + ((long long)(ch >> 3) * HW + pix) * 8 + (ch & 7)];
    if (shuffle)
      out[(((long long)n * 3 + c) * (H * s) + (y * s + sub / s)) * (long long)(W * s) + (x * s + sub % s)] = acc;
    else
      out[((long long)n * 3 * s2 + ch) * HW + pix] = acc;
  }
}

}  // namespace

extern "C" size_t sr_duf_conv3d_packed_floats(int cout, int cin, int kt) {
  if (!conv3d_served(cout, cin, kt)) return 0;
  const int gc = 16 * conv3d_ct(cout);
  return (size_t)(image_weight_floats(cout, cin, kt, 9, gc) + (cout + gc - 1) / gc * gc);
}

extern "C" int sr_duf_conv3d_pack_f32(const float* weight, const float* bias, int cout, int cin, int kt, float* packed, void* stream_) {
  SR_CHECK_ARG(conv3d_served(cout, cin, kt),
               "sr_duf_conv3d_pack_f32: (cin, cout, kt) = (%d, %d, %d) is not supported; supported: cin 3 or a multiple of 8 up to 448, "
               "cout 16 / 32 / 64 / 256, kt 1 / 3", cin, cout, kt);
  return pack_common("sr_duf_conv3d_pack_f32", weight, bias, cout, cin, kt, 9, 16 * conv3d_ct(cout), packed, (hipStream_t)stream_);
}

extern "C" int sr_duf_conv3d_f32(const sr_duf_conv_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_duf_conv3d_f32: null descriptor");
  SR_CHECK_ARG(conv3d_served(d->cout, d->cin, d->kt),
               "sr_duf_conv3d_f32: (cin, cout, kt) = (%d, %d, %d) is not supported; supported: cin 3 or a multiple of 8 up to 448, "
               "cout 16 / 32 / 64 / 256, kt 1 / 3", d->cin, d->cout, d->kt);
  SR_CHECK_ARG((d->pad_t == 0 || d->pad_t == 1) && (d->kt == 3 || d->pad_t == 0), "sr_duf_conv3d_f32: pad_t=%d does not go with kt=%d",
               d->pad_t, d->kt);
  const int ct = conv3d_ct(d->cout);
  DParams p = {};
  if (int rc = conv_common("sr_duf_conv3d_f32", d, 9, 16 * ct, p)) return rc;
  const int groups = d->cout / (16 * ct);
  if (ct == 1) return launch_conv("sr_duf_conv3d_f32 launch", duf_conv3d_f32_kernel<1>, Geo<3, 1>::LDS, p, 194, d, 9, groups, stream);
  if (ct == 2) return launch_conv("sr_duf_conv3d_f32 launch", duf_conv3d_f32_kernel<2>, Geo<3, 2>::LDS, p, 194, d, 9, groups, stream);
  return launch_conv("sr_duf_conv3d_f32 launch", duf_conv3d_f32_kernel<4>, Geo<3, 4>::LDS, p, 194, d, 9, groups, stream);
}

extern "C" size_t sr_duf_pw_packed_floats(int c) {
  if (!pw_served(c)) return 0;
  return (size_t)(image_weight_floats(c, c, 1, 1, 64) + (c + 63) / 64 * 64);
}

extern "C" int sr_duf_pw_pack_f32(const float* weight, const float* bias, int c, float* packed, void* stream_) {
  SR_CHECK_ARG(pw_served(c), "sr_duf_pw_pack_f32: c = %d is not supported; supported: a multiple of 8 up to 432", c);
  return pack_common("sr_duf_pw_pack_f32", weight, bias, c, c, 1, 1, 64, packed, (hipStream_t)stream_);
}

extern "C" int sr_duf_pw_f32(const sr_duf_conv_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(d != nullptr, "sr_duf_pw_f32: null descriptor");
  SR_CHECK_ARG(pw_served(d->cin) && d->cout == d->cin,
               "sr_duf_pw_f32: (cin, cout) = (%d, %d) is not supported; supported: cin == cout, a multiple of 8 up to 432", d->cin, d->cout);
  SR_CHECK_ARG(d->kt == 1 && d->pad_t == 0, "sr_duf_pw_f32: kt must be 1 and pad_t 0, got %d and %d", d->kt, d->pad_t);
  DParams p = {};
  if (int rc = conv_common("sr_duf_pw_f32", d, 1, 64, p)) return rc;
  return launch_conv("sr_duf_pw_f32 launch", duf_pw_f32_kernel, Geo<1, 4>::LDS, p, 196, d, 1, (d->cout + 63) / 64, stream);
}

extern "C" int sr_duf_filter_f32(const float* logits, long long logits_img_stride, const float* res, long long res_img_stride,
                                 const float* centre, long long centre_img_stride, float* out, int n, int s, int h, int w, int softmax,
                                 int shuffle, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(logits && centre && out, "sr_duf_filter_f32: null logits / centre / out");
  SR_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0, "sr_duf_filter_f32: bad shape n=%d h=%d w=%d", n, h, w);
  SR_CHECK_ARG(s >= 2 && s <= 4, "sr_duf_filter_f32: scale %d is not supported; supported: 2, 3, 4", s);
  SR_CHECK_ARG((softmax == 0 || softmax == 1) && (shuffle == 0 || shuffle == 1), "sr_duf_filter_f32: softmax and shuffle must be 0 or 1");
  const long long hw = (long long)h * w;
  const int s2 = s * s, lb = (25 * s2 + 7) / 8, rb = (3 * s2 + 7) / 8;
  SR_CHECK_ARG(hw < (1ll << 31) / (32 * lb), "sr_duf_filter_f32: image too large for 32-bit plane offsets");
  SR_CHECK_ARG(sr::aligned16(logits) && sr::aligned16(res), "sr_duf_filter_f32: CB8 tensors must be 16-byte aligned");
  SR_CHECK_ARG(logits_img_stride % 4 == 0 && (!res || res_img_stride % 4 == 0), "sr_duf_filter_f32: CB8 image strides must be multiples of 4 floats");
  SR_CHECK_ARG(logits_img_stride >= hw * 8 * lb && (!res || res_img_stride >= hw * 8 * rb) && centre_img_stride >= hw * 3,
               "sr_duf_filter_f32: an image stride is smaller than the image");
  const bool prof = sr::prof_on();
  if (prof) sr::prof_rec(stream, 197, 25 * s2, 3 * s2, n, h, w, (double)n * hw * s2 * (4.0 * 25 + 6.0 * 25), 4.0 * n * hw * (25.0 * s2 + 6.0 * s2 + 3.0));
  hipLaunchKernelGGL(duf_filter_f32_kernel, dim3((unsigned)((hw * s2 + 255) / 256), 1, (unsigned)n), dim3(256), 0, stream, logits,
                     logits_img_stride, res, res_img_stride, centre, centre_img_stride, out, s, h, w, softmax, shuffle);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_duf_filter_f32 launch");
  return SR_OK;
}
