// Channel attention of RCAN (basicsr/archs/rcan_arch.py:8-46) on CB16 bf16 activations, forward only (include/sr_hip_ca_bf16.h):
//   p[n][c] = mean_hw u[n][c],  h = relu(W1 p + b1),  s = sigmoid(W2 h + b2),  out = bf16(x + res_scale * (u * s))
// The bf16 twins of channel_attention.hip's squeeze and excite, with the same two-stage pool: one workgroup per (image, channel
// block, band of kBandPixels pixels) writes a partial per channel, and a per-image finish sums the bands in order and runs the
// MLP in fp32 on the fp32 parameters.  No atomics: every launch is bit-reproducible.  A CB16 pixel is 32 bytes; a lane always
// moves a 16-byte half of it (8 channels), so consecutive lanes cover consecutive 16 bytes of a channel-block plane.
#include "sr_internal.h"
#include "../../include/sr_hip_ca_bf16.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPoolThreads = 512;   // 256 pixels x 2 halves per step
constexpr int kBandPixels = 2048;   // pixels per partial: 8 half pixels per lane (the band of channel_attention.hip)
constexpr int kPoolSteps = kBandPixels / (kPoolThreads / 2);
constexpr int kThreads = 256;
constexpr int kExciteItems = 4;     // half pixels per lane of the excite, kThreads apart
constexpr int kMaxFeat = 512;

long long bands_of(long long hw) { return (hw + kBandPixels - 1) / kBandPixels; }

// Two floats to a bf16 pair, round to nearest even: the conversion of conv_bf16.hip's epilogue (f2bf2).
__device__ __forceinline__ unsigned f2bf2(float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  bf16x2 t = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, t);
}

// part[((n*CB + cb)*bands + band)*16 + c] = sum over the band's pixels of u[n][cb][pixel][c].  Lane t holds half (t & 1) of the
// pixels (t >> 1) + 256 i; it sums its (at most 8) half pixels in order, the 32 lanes of a wave with the same half combine by a
// fixed butterfly, and the eight waves are added in order.
__global__ __launch_bounds__(kPoolThreads) void attn16_pool_kernel(const __bf16* __restrict__ u, long long u_ns, int CB, long long HW,
                                                                   int bands, float* __restrict__ part) {
  __shared__ float red[kPoolThreads / 64][16];
  const int band = blockIdx.x, ncb = blockIdx.y;
  const int n = ncb / CB, cb = ncb - n * CB;
  const long long p0 = (long long)band * kBandPixels;
  const long long p1 = min(HW, p0 + kBandPixels);
  const int half = threadIdx.x & 1;
  const __bf16* src = u + n * u_ns + (long long)cb * HW * 16 + half * 8;
  const long long pix = p0 + (threadIdx.x >> 1);
  bf16x8_t v[kPoolSteps];
#pragma unroll
  for (int i = 0; i < kPoolSteps; ++i) {  // every load is issued before the first add
    const long long p = pix + (long long)i * (kPoolThreads / 2);
    v[i] = bf16x8_t{};
    if (p < p1) v[i] = *(const bf16x8_t*)(src + p * 16);
  }
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < kPoolSteps; ++i) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += (float)v[i][k];   // (+0 for a pixel past the band's end: exact)
  }
#pragma unroll
  for (int off = 32; off > 1; off >>= 1) {   // lanes of equal parity: the half is kept apart
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane < 2) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wave][lane * 8 + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    float t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kPoolThreads / 64; ++w) t += red[w][threadIdx.x];
    part[((long long)ncb * bands + band) * 16 + threadIdx.x] = t;
  }
}

__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }

// One workgroup per image: p = (sum of the band partials in band order) / HW, h = relu(W1 p + b1), s = sigmoid(W2 h + b2).
// W1 [hid][nf], W2 [nf][hid] (the 1x1 conv weights as stored).  Dot products run in channel order.  p_out / h_out may be null.
__global__ __launch_bounds__(kThreads) void attn16_finish_kernel(const float* __restrict__ part, int CB, int bands, float hw_den,
                                                                 const float* __restrict__ w1, const float* __restrict__ b1,
                                                                 const float* __restrict__ w2, const float* __restrict__ b2, int nf,
                                                                 int hid, float* __restrict__ p_out, float* __restrict__ h_out,
                                                                 float* __restrict__ s_out) {
  __shared__ float sp[kMaxFeat], sh[kMaxFeat];
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < nf; c += kThreads) {
    const float* q = part + ((long long)(n * CB + (c >> 4)) * bands) * 16 + (c & 15);
    float t = 0.f;
    for (int b = 0; b < bands; ++b) t += q[(long long)b * 16];
    const float p = t / hw_den;
    sp[c] = p;
    if (p_out) p_out[(long long)n * nf + c] = p;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < hid; j += kThreads) {
    const float* wr = w1 + (long long)j * nf;
    float z = 0.f;
    for (int c = 0; c < nf; ++c) z += wr[c] * sp[c];
    z += b1[j];
    const float hv = z > 0.f ? z : 0.f;
    sh[j] = hv;
    if (h_out) h_out[(long long)n * hid + j] = hv;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nf; c += kThreads) {
    const float* wr = w2 + (long long)c * hid;
    float z = 0.f;
    for (int j = 0; j < hid; ++j) z += wr[j] * sh[j];
    z += b2[c];
    s_out[(long long)n * nf + c] = sigmoidf(z);
  }
}

// out = bf16(x + rs * (u * s[n][c])) (the reference's order: CA output, then the scale, then the identity), one rounding.  An
// item is a 16-byte half pixel of one (image, channel block) plane; a workgroup takes kExciteItems * kThreads consecutive items
// and every lane issues all its loads before the first store.  out may be x: an item is read and written by the same lane only.
__global__ __launch_bounds__(kThreads) void attn16_excite_kernel(const __bf16* x, long long x_ns, const __bf16* __restrict__ u,
                                                                 long long u_ns, const float* __restrict__ s, __bf16* out, long long o_ns,
                                                                 int CB, int nf, long long items, float rs) {
  const int ncb = blockIdx.y, n = ncb / CB, cb = ncb - n * CB;
  const long long plane = (long long)cb * items * 8;
  const long long it0 = (long long)blockIdx.x * (kExciteItems * kThreads) + threadIdx.x;
  // kThreads is even, so every item of a lane is the same half of its pixel: one pair of gate vectors per lane
  const f32x4* sc = (const f32x4*)(s + (long long)n * nf + cb * 16 + (threadIdx.x & 1) * 8);
  const f32x4 sa = sc[0], sb = sc[1];
  const __bf16* px = x + n * x_ns + plane;
  const __bf16* pu = u + n * u_ns + plane;
  __bf16* po = out + n * o_ns + plane;
  bf16x8_t xv[kExciteItems], uv[kExciteItems];
#pragma unroll
  for (int i = 0; i < kExciteItems; ++i) {
    const long long it = it0 + (long long)i * kThreads;
    if (it < items) {
      xv[i] = *(const bf16x8_t*)(px + it * 8);
      uv[i] = *(const bf16x8_t*)(pu + it * 8);
    }
  }
#pragma unroll
  for (int i = 0; i < kExciteItems; ++i) {
    const long long it = it0 + (long long)i * kThreads;
    if (it >= items) continue;
    float r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float g = k < 4 ? sa[k] : sb[k - 4];
      r[k] = (float)xv[i][k] + ((float)uv[i][k] * g) * rs;
    }
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 o = {f2bf2(r[0], r[1]), f2bf2(r[2], r[3]), f2bf2(r[4], r[5]), f2bf2(r[6], r[7])};
    *(u32x4*)(po + it * 8) = o;
  }
}

void record(hipStream_t stream, int id, int c, int n, int h, int w, double bytes) {
  sr_launch_record r = {};
  r.kernel_id = id;
  r.cin = c;
  r.cout = c;
  r.n = n;
  r.h = h;
  r.w = w;
  r.bytes = bytes;
  sr::prof_begin(stream, r);
}

size_t partial_floats(int n, int nf, int h, int w) { return (size_t)n * (nf / 16) * bands_of((long long)h * w) * 16; }

// The one predicate of both entry points and of the workspace query: the shape, and that it fits one launch.
bool shape_ok(int n, int nf, int h, int w) {
  return n > 0 && h > 0 && w > 0 && nf > 0 && nf % 16 == 0 && nf <= kMaxFeat && (long long)n * (nf / 16) <= 65535 &&
         (long long)h * w < (1LL << 36);
}

// Shape and CB16 tensor checks shared by both entry points.
#define CA16_CHECK_SHAPE(who)                                                                                                      \
  SR_CHECK_ARG(shape_ok(n, nf, h, w), "%s: bad shape n=%d nf=%d %dx%d (nf a multiple of 16, at most %d; n * nf / 16 at most "       \
               "65535)", who, n, nf, h, w, kMaxFeat)

#define CA16_CHECK_CB16(who, name, ptr, ns)                                                                                        \
  SR_CHECK_ARG((ptr) != nullptr && ((uintptr_t)(ptr) % 16) == 0 && (ns) % 8 == 0, "%s: %s must be a 16-byte aligned device "       \
               "pointer with an image stride that is a multiple of 8", who, name);                                                 \
  SR_CHECK_ARG((ns) >= (long long)nf * h * w, "%s: %s image stride %lld below %lld", who, name, (long long)(ns), (long long)nf * h * w)

}  // namespace

extern "C" size_t sr_ca_workspace_bytes_bf16(int n, int nf, int hid, int h, int w) {
  if (!shape_ok(n, nf, h, w) || hid < 1 || hid > nf) return 0;
  return sr::align_up(partial_floats(n, nf, h, w), 64) * sizeof(float);
}

extern "C" int sr_ca_squeeze_bf16(const void* u, int64_t u_img_stride, int n, int nf, int h, int w, const float* w1, const float* b1,
                                  const float* w2, const float* b2, int hid, float* p, float* hbuf, float* s, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
  const char* who = "sr_ca_squeeze_bf16";
  hipStream_t stream = (hipStream_t)stream_;
  CA16_CHECK_SHAPE(who);
  SR_CHECK_ARG(hid >= 1 && hid <= nf, "%s: hidden width %d must lie in [1, nf=%d]", who, hid, nf);
  CA16_CHECK_CB16(who, "u", u, u_img_stride);
  SR_CHECK_ARG(w1 && b1 && w2 && b2 && s, "%s: null pointer", who);
  const size_t need = sr::align_up(partial_floats(n, nf, h, w), 64) * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    sr::set_error("%s: workspace of %zu bytes, needs %zu (sr_ca_workspace_bytes_bf16)", who, workspace_bytes, need);
    return SR_ENOSPACE;
  }
  const long long HW = (long long)h * w;
  const int CB = nf / 16, bands = (int)bands_of(HW);
  float* part = (float*)workspace;
  const bool prof = sr::prof_on();
  if (prof) record(stream, 102, nf, n, h, w, 2.0 * n * nf * HW + 4.0 * (double)partial_floats(n, nf, h, w));
  hipLaunchKernelGGL(attn16_pool_kernel, dim3(bands, n * CB), dim3(kPoolThreads), 0, stream, (const __bf16*)u,
                     (long long)u_img_stride, CB, HW, bands, part);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  if (prof) record(stream, 103, nf, n, 1, 1, 4.0 * ((double)partial_floats(n, nf, h, w) + 2.0 * nf * hid + n * (2.0 * nf + hid)));
  hipLaunchKernelGGL(attn16_finish_kernel, dim3(n), dim3(kThreads), 0, stream, part, CB, bands, (float)HW, w1, b1, w2, b2, nf, hid, p,
                     hbuf, s);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}

extern "C" int sr_ca_excite_bf16(const void* x, int64_t x_img_stride, const void* u, int64_t u_img_stride, const float* s, void* out,
                                 int64_t out_img_stride, int n, int nf, int h, int w, float res_scale, void* stream_) {
  const char* who = "sr_ca_excite_bf16";
  hipStream_t stream = (hipStream_t)stream_;
  CA16_CHECK_SHAPE(who);
  CA16_CHECK_CB16(who, "x", x, x_img_stride);
  CA16_CHECK_CB16(who, "u", u, u_img_stride);
  CA16_CHECK_CB16(who, "out", out, out_img_stride);
  SR_CHECK_ARG(s != nullptr && ((uintptr_t)s % 16) == 0, "%s: s must be a 16-byte aligned device pointer", who);
  const long long HW = (long long)h * w, items = 2 * HW;
  const int CB = nf / 16;
  const long long per = (long long)kExciteItems * kThreads;
  const bool prof = sr::prof_on();
  if (prof) record(stream, 104, nf, n, h, w, 2.0 * 3.0 * n * nf * HW);
  hipLaunchKernelGGL(attn16_excite_kernel, dim3((unsigned)((items + per - 1) / per), n * CB), dim3(kThreads), 0, stream,
                     (const __bf16*)x, (long long)x_img_stride, (const __bf16*)u, (long long)u_img_stride, s, (__bf16*)out,
                     (long long)out_img_stride, CB, nf, items, res_scale);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}
