// Channel attention of RCAN (basicsr/archs/rcan_arch.py:8-46), fp32 on CB8 activations:
//   p[n][c] = mean_hw u[n][c],  h = relu(W1 p + b1),  s = sigmoid(W2 h + b2),  out = x + res_scale * (u * s)
// and its adjoint.  The two reductions over the image (the pool, and sum_hw g*u in the backward) run in two stages: one
// workgroup per (image, channel block, band of kBandPixels pixels) writes a partial per channel, and a per-image finish sums
// the bands in order and runs the tiny MLP (or its adjoint).  No atomics anywhere: every launch is bit-reproducible.
// The weight gradients of W1 / b1 / W2 / b2 take one thread per element, summing the batch in order.
// The two streaming passes (excite, backward apply) move whole 32-byte CB8 pixels as two 16-byte loads / stores per tensor.
#include "sr_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBandPixels = 2048;  // pixels per partial: 8 per thread
constexpr int kMaxFeat = 512;

long long bands_of(long long hw) { return (hw + kBandPixels - 1) / kBandPixels; }

// part[((n*CB + cb)*bands + band)*8 + k] = sum over the band's pixels of a[k] (DOT = false) or a[k]*b[k] (DOT = true).
// Each thread sums its pixels in order; the 256 threads then combine by a fixed butterfly within the wave and in order across
// the four waves.
template <bool DOT>
__global__ __launch_bounds__(kThreads) void ca_partial_kernel(const float* __restrict__ a, long long a_ns, const float* __restrict__ b,
                                                              long long b_ns, int CB, long long HW, int bands,
                                                              float* __restrict__ part) {
  __shared__ float red[kThreads / 64][8];
  const int band = blockIdx.x, ncb = blockIdx.y;
  const int n = ncb / CB, cb = ncb - n * CB;
  const long long p0 = (long long)band * kBandPixels;
  const long long p1 = min(HW, p0 + kBandPixels);
  const f32x4* pa = (const f32x4*)(a + n * a_ns + (long long)cb * HW * 8);
  const f32x4* pb = DOT ? (const f32x4*)(b + n * b_ns + (long long)cb * HW * 8) : nullptr;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  for (long long p = p0 + threadIdx.x; p < p1; p += kThreads) {
    const f32x4 x0 = pa[2 * p], x1 = pa[2 * p + 1];
    if (DOT) {
      const f32x4 y0 = pb[2 * p], y1 = pb[2 * p + 1];
      s0 += x0 * y0;
      s1 += x1 * y1;
    } else {
      s0 += x0;
      s1 += x1;
    }
  }
  float v[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += __shfl_xor(v[k], off, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    float t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) t += red[w][threadIdx.x];
    part[((long long)ncb * bands + band) * 8 + threadIdx.x] = t;
  }
}

// Sum of channel c's band partials, in band order.
__device__ __forceinline__ float band_sum(const float* part, int n, int c, int CB, int bands) {
  const float* q = part + ((long long)(n * CB + (c >> 3)) * bands) * 8 + (c & 7);
  float t = 0.f;
  for (int b = 0; b < bands; ++b) t += q[b * 8];
  return t;
}

__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }

// One workgroup per image: p = pool, h = relu(W1 p + b1), s = sigmoid(W2 h + b2).  W1 [hid][nf], W2 [nf][hid] (the 1x1 conv
// weights as stored).  Dot products run in channel order.
__global__ __launch_bounds__(kThreads) void ca_squeeze_finish_kernel(const float* __restrict__ part, int CB, int bands, float hw_den,
                                                                     const float* __restrict__ w1, const float* __restrict__ b1,
                                                                     const float* __restrict__ w2, const float* __restrict__ b2, int nf,
                                                                     int hid, float* __restrict__ p_out, float* __restrict__ h_out,
                                                                     float* __restrict__ s_out) {
  __shared__ float sp[kMaxFeat], sh[kMaxFeat];
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < nf; c += kThreads) {
    const float p = band_sum(part, n, c, CB, bands) / hw_den;
    sp[c] = p;
    p_out[(long long)n * nf + c] = p;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < hid; j += kThreads) {
    const float* wr = w1 + (long long)j * nf;
    float z = 0.f;
    for (int c = 0; c < nf; ++c) z += wr[c] * sp[c];
    z += b1[j];
    const float hv = z > 0.f ? z : 0.f;
    sh[j] = hv;
    h_out[(long long)n * hid + j] = hv;
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

// out = x + res_scale * (u * s[n][c]) (the reference's order: CA output, then the scale, then the identity).  One thread per
// CB8 pixel.  out may be x (in place).
__global__ __launch_bounds__(kThreads) void ca_excite_kernel(const float* x, long long x_ns, const float* __restrict__ u, long long u_ns,
                                                             const float* __restrict__ s, float* out, long long o_ns, int CB, int nf,
                                                             long long HW, float rs) {
  const long long pix = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (pix >= HW) return;
  const int ncb = blockIdx.y, n = ncb / CB, cb = ncb - n * CB;
  const long long off = ((long long)cb * HW + pix) * 8;
  const float* sc = s + (long long)n * nf + cb * 8;
  const f32x4 sa = {sc[0], sc[1], sc[2], sc[3]}, sb = {sc[4], sc[5], sc[6], sc[7]};
  const f32x4* pu = (const f32x4*)(u + n * u_ns + off);
  const f32x4* px = (const f32x4*)(x + n * x_ns + off);
  const f32x4 u0 = pu[0], u1 = pu[1], x0 = px[0], x1 = px[1];
  f32x4* po = (f32x4*)(out + n * o_ns + off);
  po[0] = x0 + (u0 * sa) * rs;
  po[1] = x1 + (u1 * sb) * rs;
}

// One workgroup per image, the adjoint of the squeeze: ds = res_scale * sum_hw g*u, dz2 = ds * s(1 - s), dh = W2^T dz2,
// dz1 = dh where h > 0, dp = W1^T dz1, q = dp / (H*W).  dz2 / dz1 go to the workspace for the weight-gradient launch.
__global__ __launch_bounds__(kThreads) void ca_bwd_finish_kernel(const float* __restrict__ part, int CB, int bands, float rs, float hw_den,
                                                                 const float* __restrict__ w1, const float* __restrict__ w2,
                                                                 const float* __restrict__ h_in, const float* __restrict__ s_in, int nf,
                                                                 int hid, float* __restrict__ dz2_out, float* __restrict__ dz1_out,
                                                                 float* __restrict__ q_out) {
  __shared__ float sz2[kMaxFeat], sz1[kMaxFeat];
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < nf; c += kThreads) {
    const float ds = rs * band_sum(part, n, c, CB, bands);
    const float s = s_in[(long long)n * nf + c];
    const float dz = ds * ((1.f - s) * s);
    sz2[c] = dz;
    dz2_out[(long long)n * nf + c] = dz;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < hid; j += kThreads) {
    float dh = 0.f;
    for (int c = 0; c < nf; ++c) dh += w2[(long long)c * hid + j] * sz2[c];
    const float dz = h_in[(long long)n * hid + j] > 0.f ? dh : 0.f;
    sz1[j] = dz;
    dz1_out[(long long)n * hid + j] = dz;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nf; c += kThreads) {
    float dp = 0.f;
    for (int j = 0; j < hid; ++j) dp += w1[(long long)j * nf + c] * sz1[j];
    q_out[(long long)n * nf + c] = dp / hw_den;
  }
}

// dW1[j][c] = sum_n dz1[n][j] p[n][c], db1[j] = sum_n dz1[n][j], dW2[c][j] = sum_n dz2[n][c] h[n][j], db2[c] = sum_n dz2[n][c]:
// one thread per element, the batch summed in order.  A null destination is skipped; accumulate = 1 adds into it.
__global__ __launch_bounds__(kThreads) void ca_wgrad_kernel(const float* __restrict__ dz1, const float* __restrict__ dz2,
                                                            const float* __restrict__ p, const float* __restrict__ h, int n, int nf,
                                                            int hid, float* dw1, float* db1, float* dw2, float* db2, int accumulate) {
  long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long n_w = (long long)nf * hid;
  float acc = 0.f;
  float* dst;
  if (e < n_w) {
    if (!dw1) return;
    const int j = (int)(e / nf), c = (int)(e - (long long)j * nf);
    for (int i = 0; i < n; ++i) acc += dz1[(long long)i * hid + j] * p[(long long)i * nf + c];
    dst = dw1 + e;
  } else if ((e -= n_w) < hid) {
    if (!db1) return;
    for (int i = 0; i < n; ++i) acc += dz1[(long long)i * hid + e];
    dst = db1 + e;
  } else if ((e -= hid) < n_w) {
    if (!dw2) return;
    const int c = (int)(e / hid), j = (int)(e - (long long)c * hid);
    for (int i = 0; i < n; ++i) acc += dz2[(long long)i * nf + c] * h[(long long)i * hid + j];
    dst = dw2 + e;
  } else if ((e -= n_w) < nf) {
    if (!db2) return;
    for (int i = 0; i < n; ++i) acc += dz2[(long long)i * nf + e];
    dst = db2 + e;
  } else {
    return;
  }
  *dst = accumulate ? *dst + acc : acc;
}

// du = (res_scale * g) * s[n][c] + q[n][c]: the direct path of u * s plus the pool's (spread) gradient.  du may be g (in place).
__global__ __launch_bounds__(kThreads) void ca_bwd_apply_kernel(const float* g, long long g_ns, const float* __restrict__ s,
                                                                const float* __restrict__ q, float* du, long long d_ns, int CB, int nf,
                                                                long long HW, float rs) {
  const long long pix = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (pix >= HW) return;
  const int ncb = blockIdx.y, n = ncb / CB, cb = ncb - n * CB;
  const long long off = ((long long)cb * HW + pix) * 8;
  const float* sc = s + (long long)n * nf + cb * 8;
  const float* qc = q + (long long)n * nf + cb * 8;
  const f32x4 sa = {sc[0], sc[1], sc[2], sc[3]}, sb = {sc[4], sc[5], sc[6], sc[7]};
  const f32x4 qa = {qc[0], qc[1], qc[2], qc[3]}, qb = {qc[4], qc[5], qc[6], qc[7]};
  const f32x4* pg = (const f32x4*)(g + n * g_ns + off);
  const f32x4 g0 = pg[0], g1 = pg[1];
  f32x4* pd = (f32x4*)(du + n * d_ns + off);
  pd[0] = (g0 * rs) * sa + qa;
  pd[1] = (g1 * rs) * sb + qb;
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

size_t partial_floats(int n, int nf, int h, int w) { return (size_t)n * (nf / 8) * bands_of((long long)h * w) * 8; }

size_t workspace_floats(int n, int nf, int hid, int h, int w) {
  return sr::align_up(partial_floats(n, nf, h, w), 64) + sr::align_up((size_t)n * nf, 64) + sr::align_up((size_t)n * hid, 64);
}

// Shape and CB8 tensor checks shared by every entry point.
#define CA_CHECK_SHAPE(who)                                                                                                           \
  SR_CHECK_ARG(n > 0 && h > 0 && w > 0 && nf > 0 && nf % 8 == 0 && nf <= kMaxFeat, "%s: bad shape n=%d nf=%d %dx%d (nf a multiple " \
               "of 8, at most %d)", who, n, nf, h, w, kMaxFeat);                                                                     \
  SR_CHECK_ARG((long long)n * (nf / 8) <= 65535 && (long long)h * w / kThreads < (1LL << 31) - 1, "%s: n=%d nf=%d %dx%d exceeds one " \
               "launch", who, n, nf, h, w)

#define CA_CHECK_CB8(who, name, ptr, ns)                                                                                            \
  SR_CHECK_ARG((ptr) != nullptr && ((uintptr_t)(ptr) % 16) == 0, "%s: %s must be a 16-byte aligned device pointer", who, name);     \
  SR_CHECK_ARG((ns) >= (long long)(nf / 8) * h * w * 8, "%s: %s image stride %lld below %lld", who, name, (long long)(ns),           \
               (long long)(nf / 8) * h * w * 8)

}  // namespace

extern "C" size_t sr_ca_workspace_bytes(int n, int nf, int hid, int h, int w) {
  if (n <= 0 || nf <= 0 || nf % 8 || hid <= 0 || h <= 0 || w <= 0) return 0;
  return workspace_floats(n, nf, hid, h, w) * sizeof(float);
}

extern "C" int sr_ca_squeeze_f32(const float* u, int64_t u_img_stride, int n, int nf, int h, int w, const float* w1, const float* b1,
                                 const float* w2, const float* b2, int hid, float* p, float* hbuf, float* s, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
  const char* who = "sr_ca_squeeze_f32";
  hipStream_t stream = (hipStream_t)stream_;
  CA_CHECK_SHAPE(who);
  SR_CHECK_ARG(hid >= 1 && hid <= nf, "%s: hidden width %d must lie in [1, nf=%d]", who, hid, nf);
  CA_CHECK_CB8(who, "u", u, u_img_stride);
  SR_CHECK_ARG(w1 && b1 && w2 && b2 && p && hbuf && s, "%s: null pointer", who);
  const size_t need = workspace_floats(n, nf, hid, h, w) * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    sr::set_error("%s: workspace of %zu bytes, needs %zu (sr_ca_workspace_bytes)", who, workspace_bytes, need);
    return SR_ENOSPACE;
  }
  const long long HW = (long long)h * w;
  const int CB = nf / 8, bands = (int)bands_of(HW);
  float* part = (float*)workspace;
  const bool prof = sr::prof_on();
  if (prof) record(stream, 74, nf, n, h, w, 4.0 * ((double)n * nf * HW + (double)partial_floats(n, nf, h, w)));
  hipLaunchKernelGGL(ca_partial_kernel<false>, dim3(bands, n * CB), dim3(kThreads), 0, stream, u, (long long)u_img_stride, nullptr,
                     0LL, CB, HW, bands, part);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  if (prof) record(stream, 75, nf, n, 1, 1, 4.0 * ((double)partial_floats(n, nf, h, w) + 2.0 * nf * hid + n * (2.0 * nf + hid)));
  hipLaunchKernelGGL(ca_squeeze_finish_kernel, dim3(n), dim3(kThreads), 0, stream, part, CB, bands, (float)HW, w1, b1, w2, b2, nf, hid,
                     p, hbuf, s);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}

extern "C" int sr_ca_excite_f32(const float* x, int64_t x_img_stride, const float* u, int64_t u_img_stride, const float* s, float* out,
                                int64_t out_img_stride, int n, int nf, int h, int w, float res_scale, void* stream_) {
  const char* who = "sr_ca_excite_f32";
  hipStream_t stream = (hipStream_t)stream_;
  CA_CHECK_SHAPE(who);
  CA_CHECK_CB8(who, "x", x, x_img_stride);
  CA_CHECK_CB8(who, "u", u, u_img_stride);
  CA_CHECK_CB8(who, "out", out, out_img_stride);
  SR_CHECK_ARG(s != nullptr, "%s: null pointer", who);
  const long long HW = (long long)h * w;
  const int CB = nf / 8;
  const bool prof = sr::prof_on();
  if (prof) record(stream, 76, nf, n, h, w, 4.0 * 3.0 * n * nf * HW);
  hipLaunchKernelGGL(ca_excite_kernel, dim3((unsigned)((HW + kThreads - 1) / kThreads), n * CB), dim3(kThreads), 0, stream, x,
                     (long long)x_img_stride, u, (long long)u_img_stride, s, out, (long long)out_img_stride, CB, nf, HW, res_scale);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}

extern "C" int sr_ca_bwd_f32(const float* g, int64_t g_img_stride, const float* u, int64_t u_img_stride, int n, int nf, int h, int w,
                             float res_scale, const float* w1, const float* w2, int hid, const float* p, const float* hbuf,
                             const float* s, float* dw1, float* db1, float* dw2, float* db2, int accumulate, float* q, void* workspace,
                             size_t workspace_bytes, void* stream_) {
  const char* who = "sr_ca_bwd_f32";
  hipStream_t stream = (hipStream_t)stream_;
  CA_CHECK_SHAPE(who);
  SR_CHECK_ARG(hid >= 1 && hid <= nf, "%s: hidden width %d must lie in [1, nf=%d]", who, hid, nf);
  CA_CHECK_CB8(who, "g", g, g_img_stride);
  CA_CHECK_CB8(who, "u", u, u_img_stride);
  SR_CHECK_ARG(w1 && w2 && p && hbuf && s && q, "%s: null pointer", who);
  const size_t need = workspace_floats(n, nf, hid, h, w) * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    sr::set_error("%s: workspace of %zu bytes, needs %zu (sr_ca_workspace_bytes)", who, workspace_bytes, need);
    return SR_ENOSPACE;
  }
  const long long HW = (long long)h * w;
  const int CB = nf / 8, bands = (int)bands_of(HW);
  float* part = (float*)workspace;
  float* dz2 = part + sr::align_up(partial_floats(n, nf, h, w), 64);
  float* dz1 = dz2 + sr::align_up((size_t)n * nf, 64);
  const bool prof = sr::prof_on();
  if (prof) record(stream, 77, nf, n, h, w, 4.0 * (2.0 * n * nf * HW + (double)partial_floats(n, nf, h, w)));
  hipLaunchKernelGGL(ca_partial_kernel<true>, dim3(bands, n * CB), dim3(kThreads), 0, stream, g, (long long)g_img_stride, u,
                     (long long)u_img_stride, CB, HW, bands, part);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  if (prof) record(stream, 78, nf, n, 1, 1, 4.0 * ((double)partial_floats(n, nf, h, w) + 2.0 * nf * hid + n * (4.0 * nf + 2.0 * hid)));
  hipLaunchKernelGGL(ca_bwd_finish_kernel, dim3(n), dim3(kThreads), 0, stream, part, CB, bands, res_scale, (float)HW, w1, w2, hbuf, s,
                     nf, hid, dz2, dz1, q);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  if (dw1 || db1 || dw2 || db2) {
    const long long total = 2LL * nf * hid + nf + hid;
    if (prof) record(stream, 79, nf, n, 1, 1, 4.0 * ((double)n * (2.0 * nf + 2.0 * hid) + (1.0 + accumulate) * total));
    hipLaunchKernelGGL(ca_wgrad_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, dz1, dz2, p,
                       hbuf, n, nf, hid, dw1, db1, dw2, db2, accumulate);
    if (prof) sr::prof_end(stream);
    SR_CHECK_LAUNCH(who);
  }
  return SR_OK;
}

extern "C" int sr_ca_bwd_apply_f32(const float* g, int64_t g_img_stride, const float* s, const float* q, float* du,
                                   int64_t du_img_stride, int n, int nf, int h, int w, float res_scale, void* stream_) {
  const char* who = "sr_ca_bwd_apply_f32";
  hipStream_t stream = (hipStream_t)stream_;
  CA_CHECK_SHAPE(who);
  CA_CHECK_CB8(who, "g", g, g_img_stride);
  CA_CHECK_CB8(who, "du", du, du_img_stride);
  SR_CHECK_ARG(s && q, "%s: null pointer", who);
  const long long HW = (long long)h * w;
  const int CB = nf / 8;
  const bool prof = sr::prof_on();
  if (prof) record(stream, 80, nf, n, h, w, 4.0 * 2.0 * n * nf * HW);
  hipLaunchKernelGGL(ca_bwd_apply_kernel, dim3((unsigned)((HW + kThreads - 1) / kThreads), n * CB), dim3(kThreads), 0, stream, g,
                     (long long)g_img_stride, s, q, du, (long long)du_img_stride, CB, nf, HW, res_scale);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH(who);
  return SR_OK;
}
