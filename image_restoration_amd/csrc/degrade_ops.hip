// The degradation chain of the reference's plate training set on the device (include/sr_hip_degrade.h): blur, bilinear resize,
// Gaussian noise, DiffJPEG (forward and backward) and the tail of the dataset's __getitem__.
//
// Reference, per sample on host cores (basicsr/data/ocr_degradation_dataset.py:229-288): cv2.filter2D with a drawn kernel,
// cv2.resize down by a drawn factor, numpy noise, a libjpeg round trip, cv2.resize back, jitter / gray / round / normalise; the
// tensor forms of the same steps are utils/img_process_util.py:filter2D, data/degradations.py:add_gaussian_noise_pt and
// utils/diffjpeg.py:DiffJPEG.  Here the host only draws the parameters and ships uint8 (data/device_pipeline.py); every stage
// is one launch over the batch.  All of them are HBM-bound image passes: 8 B per value for the elementwise ones, the source
// window read once through LDS for the blur, one read and one write per pixel for the JPEG (its six 8x8 transforms stay in LDS).
#include <math.h>

#include "../../include/sr_hip_degrade.h"
#include "sr_internal.h"

namespace {

void prof_rec(hipStream_t stream, int id, int c, int n, int h, int w, double flops, double bytes) {
  sr_launch_record r = {};
  r.kernel_id = id;
  r.cin = c;
  r.cout = c;
  r.n = n;
  r.h = h;
  r.w = w;
  r.flops = flops;
  r.bytes = bytes;
  sr::prof_begin(stream, r);
}

// (h, w) of sample b clamped to the buffer; a null array means the whole buffer
__device__ __forceinline__ void sample_size(const int* sizes, int b, int hmax, int wmax, int& h, int& w) {
  h = hmax;
  w = wmax;
  if (sizes) {
    h = min(max(sizes[2 * b], 0), hmax);
    w = min(max(sizes[2 * b + 1], 0), wmax);
  }
}

// --------------------------------------------------------------------------------------------------------------- filter2d
constexpr int kFTileW = 64, kFTileH = 16, kFMaxK = 21;
constexpr int kFRows = kFTileH + kFMaxK - 1, kFPitch = kFTileW + kFMaxK - 1 + 1;

__device__ __forceinline__ int reflect_index(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return min(max(i, 0), n - 1);  // (only tile positions no output of the image reads get here out of range)
}

__global__ __launch_bounds__(256) void filter2d_kernel(const float* __restrict__ x, const float* __restrict__ kernels,
                                                       float* __restrict__ out, int C, int H, int W, int k, int kernel_batch) {
  __shared__ float tile[kFRows * kFPitch];
  __shared__ float kern[kFMaxK * kFMaxK];
  const int plane = blockIdx.z, b = plane / C;
  const int x0 = blockIdx.x * kFTileW, y0 = blockIdx.y * kFTileH, pad = k / 2;
  const int tw = kFTileW + k - 1, th = kFTileH + k - 1;
  const float* src = x + (long long)plane * H * W;
  const float* kp = kernels + (kernel_batch == 1 ? 0 : (long long)b * k * k);
  for (int i = threadIdx.x; i < k * k; i += 256) kern[i] = kp[i];
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const int r = i / tw, c = i - r * tw;
    const int gy = reflect_index(y0 + r - pad, H), gx = reflect_index(x0 + c - pad, W);
    tile[r * kFPitch + c] = src[(long long)gy * W + gx];
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = (threadIdx.x >> 6) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ky = 0; ky < k; ++ky)
    for (int kx = 0; kx < k; ++kx) {
      const float wv = kern[ky * k + kx];
      const float* t = tile + (ty + ky) * kFPitch + tx + kx;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(wv, t[j * kFPitch], acc[j]);
    }
  const int gx = x0 + tx;
  if (gx >= W) return;
  float* dst = out + (long long)plane * H * W;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gy = y0 + ty + j;
    if (gy < H) dst[(long long)gy * W + gx] = acc[j];
  }
}

// ----------------------------------------------------------------------------------------------------------------- resize
__device__ __forceinline__ void source_coord(int d, int src_len, float scale, int& i0, int& i1, float& f) {
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

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ src, const int* __restrict__ src_sizes,
                                                              float* __restrict__ dst, const int* __restrict__ dst_sizes, int C,
                                                              int Hs, int Ws, int Hd, int Wd) {
  const int plane = blockIdx.z, b = plane / C;
  const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (dx >= Wd || dy >= Hd) return;
  int hs, ws, hd, wd;
  sample_size(src_sizes, b, Hs, Ws, hs, ws);
  sample_size(dst_sizes, b, Hd, Wd, hd, wd);
  float v = 0.f;
  if (dy < hd && dx < wd && hs > 0 && ws > 0) {
    int y0, y1, x0, x1;
    float fy, fx;
    source_coord(dy, hs, (float)hs / (float)hd, y0, y1, fy);
    source_coord(dx, ws, (float)ws / (float)wd, x0, x1, fx);
    const float* s = src + (long long)plane * Hs * Ws;
    const double a = s[(long long)y0 * Ws + x0], bb = s[(long long)y0 * Ws + x1];
    const double c = s[(long long)y1 * Ws + x0], d = s[(long long)y1 * Ws + x1];
    const double gx = fx, gy = fy;
    v = (float)((1.0 - gy) * ((1.0 - gx) * a + gx * bb) + gy * ((1.0 - gx) * c + gx * d));
  }
  dst[((long long)plane * Hd + dy) * Wd + dx] = v;
}

// ------------------------------------------------------------------------------------------------------------------ noise
__device__ __forceinline__ float noise_value(float x, float nz, float sigma, int clip, int rounds) {
  const float n = nz * sigma / 255.f;
  float o = x + n;
  if (clip && rounds)
    o = fminf(fmaxf(rintf(o * 255.f), 0.f), 255.f) / 255.f;
  else if (clip)
    o = fminf(fmaxf(o, 0.f), 1.f);
  else if (rounds)
    o = rintf(o * 255.f) / 255.f;
  return o;
}

template <int V>
__global__ __launch_bounds__(256) void gaussian_noise_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                             const float* __restrict__ noise_gray, const float* __restrict__ sigma,
                                                             const float* __restrict__ gray, float* out, int C, long long hw,
                                                             int clip, int rounds) {
  const int b = blockIdx.z, c = blockIdx.y;
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  if (i >= hw) return;
  const float sg = sigma[b];
  const bool g = gray && gray[b] != 0.f;
  const long long off = ((long long)b * C + c) * hw + i;
  const float* nz = g ? noise_gray + (long long)b * hw + i : noise + off;
  if (V == 4) {
    const float4 xv = *(const float4*)(x + off), nv = *(const float4*)nz;
    float4 o;
    o.x = noise_value(xv.x, nv.x, sg, clip, rounds);
    o.y = noise_value(xv.y, nv.y, sg, clip, rounds);
    o.z = noise_value(xv.z, nv.z, sg, clip, rounds);
    o.w = noise_value(xv.w, nv.w, sg, clip, rounds);
    *(float4*)(out + off) = o;
  } else {
    out[off] = noise_value(x[off], nz[0], sg, clip, rounds);
  }
}

// ----------------------------------------------------------------------------------------------------------------- finish
struct FinishParams {
  const float* x;
  const float* jitter;
  const float* gray;
  float* out;
  long long hw;
  float mean[3], stdv[3];
  int normalise;
};

__device__ __forceinline__ void finish_pixel(float& r, float& g, float& b, const float* jit, bool gray, const FinishParams& p) {
  if (jit) {
    r = fminf(fmaxf(r + jit[0], 0.f), 1.f);
    g = fminf(fmaxf(g + jit[1], 0.f), 1.f);
    b = fminf(fmaxf(b + jit[2], 0.f), 1.f);
  }
  if (gray) r = g = b = (0.299f * r + 0.587f * g) + 0.114f * b;
  r = fminf(fmaxf(rintf(r * 255.f), 0.f), 255.f) / 255.f;
  g = fminf(fmaxf(rintf(g * 255.f), 0.f), 255.f) / 255.f;
  b = fminf(fmaxf(rintf(b * 255.f), 0.f), 255.f) / 255.f;
  if (p.normalise) {
    r = (r - p.mean[0]) / p.stdv[0];
    g = (g - p.mean[1]) / p.stdv[1];
    b = (b - p.mean[2]) / p.stdv[2];
  }
}

template <int V>
__global__ __launch_bounds__(256) void degrade_finish_kernel(const FinishParams p) {
  const int b = blockIdx.z;
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  if (i >= p.hw) return;
  const float* jit = p.jitter ? p.jitter + 3 * b : nullptr;
  const bool gray = p.gray && p.gray[b] != 0.f;
  const long long o0 = (long long)b * 3 * p.hw + i, o1 = o0 + p.hw, o2 = o1 + p.hw;
  if (V == 4) {
    float4 r = *(const float4*)(p.x + o0), g = *(const float4*)(p.x + o1), bl = *(const float4*)(p.x + o2);
    finish_pixel(r.x, g.x, bl.x, jit, gray, p);
    finish_pixel(r.y, g.y, bl.y, jit, gray, p);
    finish_pixel(r.z, g.z, bl.z, jit, gray, p);
    finish_pixel(r.w, g.w, bl.w, jit, gray, p);
    *(float4*)(p.out + o0) = r;
    *(float4*)(p.out + o1) = g;
    *(float4*)(p.out + o2) = bl;
  } else {
    float r = p.x[o0], g = p.x[o1], bl = p.x[o2];
    finish_pixel(r, g, bl, jit, gray, p);
    p.out[o0] = r;
    p.out[o1] = g;
    p.out[o2] = bl;
  }
}

// --------------------------------------------------------------------------------------------------------------- DiffJPEG
// cos(j pi / 16), j = 0 .. 31; C[n][k] = cos((2n + 1) k pi / 16) = kCos32[((2n + 1) k) & 31]
__constant__ float kCos32[32] = {
    1.f,           0.98078528040323f,  0.92387953251129f,  0.83146961230255f,  0.70710678118655f,  0.55557023301960f,
    0.38268343236509f,  0.19509032201613f,  0.f,           -0.19509032201613f, -0.38268343236509f, -0.55557023301960f,
    -0.70710678118655f, -0.83146961230255f, -0.92387953251129f, -0.98078528040323f, -1.f,          -0.98078528040323f,
    -0.92387953251129f, -0.83146961230255f, -0.70710678118655f, -0.55557023301960f, -0.38268343236509f, -0.19509032201613f,
    0.f,           0.19509032201613f,  0.38268343236509f,  0.55557023301960f,  0.70710678118655f,  0.83146961230255f,
    0.92387953251129f,  0.98078528040323f};
// the luminance table as the JPEG standard prints it; the reference transposes it (diffjpeg.py:18), so entry [u][v] is kYStd[v][u]
__constant__ float kYStd[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                69, 56, 14, 17, 22, 29,  51,  87,  80,  62, 18, 22, 37, 56, 68,  109, 103, 77, 24, 35, 55, 64,
                                81, 104, 113, 92, 49, 64, 78, 87,  103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
// the top-left 4x4 of the chrominance table (symmetric; the rest is 99)
__constant__ float kCStd[16] = {17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 99, 47, 66, 99, 99};

constexpr int kBP = 9;  // pitch of an 8x8 block row in LDS
struct JpegLds {
  float cosv[64];
  float pix[2][16][17];      // Cb, Cr (or their gradients) at full resolution
  float blk[6][8][kBP];      // blocks 0-3: Y (2 x 2), 4: Cb, 5: Cr
  float tmp[6][8][kBP];
  float coef[6][8][kBP];
  float dq[6][8][kBP];       // backward: q - r of every coefficient
};

__device__ __forceinline__ float dct_scale(int u, int v) {  // outer(alpha, alpha) / 4, alpha = (1 / sqrt 2, 1, .. 1)
  return (u == 0 && v == 0) ? 0.125f : (u == 0 || v == 0) ? 0.17677669529663687f : 0.25f;
}
__device__ __forceinline__ float idct_alpha(int x, int y) {  // outer(alpha, alpha)
  return (x == 0 && y == 0) ? 0.5f : (x == 0 || y == 0) ? 0.70710678118654752f : 1.f;
}
__device__ __forceinline__ float quant_table(int b, int u, int v) {
  if (b < 4) return kYStd[v * 8 + u];
  return (u < 4 && v < 4) ? kCStd[u * 4 + v] : 99.f;
}

// out[b][u][v] = alpha_u alpha_v / 4 * sum_x sum_y in[b][x][y] C[x][u] C[y][v]           (dct_8x8 without the - 128)
__device__ __forceinline__ void dct2(JpegLds& L, const float (*in)[8][kBP], float (*out)[8][kBP]) {
  for (int i = threadIdx.x; i < 384; i += 256) {
    const int b = i >> 6, x = (i >> 3) & 7, v = i & 7;
    float s = 0.f;
#pragma unroll
    for (int y = 0; y < 8; ++y) s = fmaf(in[b][x][y], L.cosv[y * 8 + v], s);
    L.tmp[b][x][v] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 384; i += 256) {
    const int b = i >> 6, u = (i >> 3) & 7, v = i & 7;
    float s = 0.f;
#pragma unroll
    for (int x = 0; x < 8; ++x) s = fmaf(L.tmp[b][x][v], L.cosv[x * 8 + u], s);
    out[b][u][v] = s * dct_scale(u, v);
  }
  __syncthreads();
}

// out[b][u][v] = 1/4 * sum_x sum_y in[b][x][y] alpha_x alpha_y C[u][x] C[v][y] + add            (idct_8x8)
__device__ __forceinline__ void idct2(JpegLds& L, const float (*in)[8][kBP], float (*out)[8][kBP], float add) {
  for (int i = threadIdx.x; i < 384; i += 256) {
    const int b = i >> 6, x = (i >> 3) & 7, v = i & 7;
    float s = 0.f;
#pragma unroll
    for (int y = 0; y < 8; ++y) s = fmaf(in[b][x][y] * idct_alpha(x, y), L.cosv[v * 8 + y], s);
    L.tmp[b][x][v] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 384; i += 256) {
    const int b = i >> 6, u = (i >> 3) & 7, v = i & 7;
    float s = 0.f;
#pragma unroll
    for (int x = 0; x < 8; ++x) s = fmaf(L.tmp[b][x][v], L.cosv[u * 8 + x], s);
    out[b][u][v] = 0.25f * s + add;
  }
  __syncthreads();
}

// 2x2 reduction of the two full-resolution planes in L.pix into blocks 4 and 5: (sum * scale) + add
__device__ __forceinline__ void chroma_pool(JpegLds& L, float scale, float add) {
  if (threadIdx.x < 128) {
    const int ch = threadIdx.x >> 6, cy = (threadIdx.x >> 3) & 7, cx = threadIdx.x & 7;
    const float s = ((L.pix[ch][2 * cy][2 * cx] + L.pix[ch][2 * cy][2 * cx + 1]) + L.pix[ch][2 * cy + 1][2 * cx]) +
                    L.pix[ch][2 * cy + 1][2 * cx + 1];
    L.blk[4 + ch][cy][cx] = s * scale + add;
  }
}

// The forward chain of one macroblock up to the values before the clamp (r, g, b of the thread's pixel, 0..255 scale); with
// KEEP_DQ the rounding residuals q - r stay in L.dq.  Ends behind a barrier; L.coef holds the decoded Y, Cb, Cr blocks.
template <bool KEEP_DQ>
__device__ __forceinline__ void jpeg_forward(JpegLds& L, float r, float g, float b, float factor, int differentiable, float& ro,
                                             float& go, float& bo) {
  const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
  if (threadIdx.x < 64) L.cosv[threadIdx.x] = kCos32[((2 * (threadIdx.x >> 3) + 1) * (threadIdx.x & 7)) & 31];
  r *= 255.f;
  g *= 255.f;
  b *= 255.f;
  const float y = (0.299f * r + 0.587f * g) + 0.114f * b;
  const float cb = ((-0.168736f * r + -0.331264f * g) + 0.5f * b) + 128.f;
  const float cr = ((0.5f * r + -0.418688f * g) + -0.081312f * b) + 128.f;
  const int yb = (py >> 3) * 2 + (px >> 3);
  L.blk[yb][py & 7][px & 7] = y - 128.f;
  L.pix[0][py][px] = cb;
  L.pix[1][py][px] = cr;
  __syncthreads();
  chroma_pool(L, 0.25f, -128.f);
  __syncthreads();
  dct2(L, L.blk, L.coef);
  for (int i = threadIdx.x; i < 384; i += 256) {
    const int bk = i >> 6, u = (i >> 3) & 7, v = i & 7;
    const float t = quant_table(bk, u, v) * factor;
    const float q = L.coef[bk][u][v] / t;
    float rq = rintf(q);
    const float d = q - rq;
    if (KEEP_DQ) L.dq[bk][u][v] = d;
    if (differentiable) rq = rq + d * d * d;
    L.blk[bk][u][v] = rq * t;
  }
  __syncthreads();
  idct2(L, L.blk, L.coef, 128.f);
  const float yy = L.coef[yb][py & 7][px & 7];
  const float cbs = L.coef[4][py >> 1][px >> 1] - 128.f, crs = L.coef[5][py >> 1][px >> 1] - 128.f;
  ro = yy + 1.402f * crs;
  go = (yy + -0.344136f * cbs) + -0.714136f * crs;
  bo = yy + 1.772f * cbs;
}

__global__ __launch_bounds__(256) void diffjpeg_kernel(const float* x, const int* __restrict__ sizes,
                                                       const float* __restrict__ factor, float* out, int H, int W,
                                                       int differentiable) {
  __shared__ JpegLds L;
  const int b = blockIdx.z, py = threadIdx.x >> 4, px = threadIdx.x & 15;
  const int gy = blockIdx.y * 16 + py, gx = blockIdx.x * 16 + px;
  int hs, ws;
  sample_size(sizes, b, H, W, hs, ws);
  const long long hw = (long long)H * W, off = (long long)b * 3 * hw + (long long)gy * W + gx;
  const bool in_buf = gy < H && gx < W, inside = gy < hs && gx < ws;
  if ((int)blockIdx.y * 16 >= hs || (int)blockIdx.x * 16 >= ws) {  // a macroblock no pixel of the sample lies in (uniform)
    if (in_buf) out[off] = out[off + hw] = out[off + 2 * hw] = 0.f;
    return;
  }
  float r = 0.f, g = 0.f, bl = 0.f;
  if (inside) {
    r = x[off];
    g = x[off + hw];
    bl = x[off + 2 * hw];
  }
  float ro, go, bo;
  jpeg_forward<false>(L, r, g, bl, factor[b], differentiable, ro, go, bo);
  if (!in_buf) return;
  out[off] = inside ? fminf(fmaxf(ro, 0.f), 255.f) / 255.f : 0.f;
  out[off + hw] = inside ? fminf(fmaxf(go, 0.f), 255.f) / 255.f : 0.f;
  out[off + 2 * hw] = inside ? fminf(fmaxf(bo, 0.f), 255.f) / 255.f : 0.f;
}

__global__ __launch_bounds__(256) void diffjpeg_bwd_kernel(const float* __restrict__ x, const int* __restrict__ sizes,
                                                           const float* __restrict__ factor, const float* grad_out, float* grad_x,
                                                           int H, int W) {
  __shared__ JpegLds L;
  const int b = blockIdx.z, py = threadIdx.x >> 4, px = threadIdx.x & 15;
  const int gy = blockIdx.y * 16 + py, gx = blockIdx.x * 16 + px;
  int hs, ws;
  sample_size(sizes, b, H, W, hs, ws);
  const long long hw = (long long)H * W, off = (long long)b * 3 * hw + (long long)gy * W + gx;
  const bool in_buf = gy < H && gx < W, inside = gy < hs && gx < ws;
  if ((int)blockIdx.y * 16 >= hs || (int)blockIdx.x * 16 >= ws) {
    if (in_buf) grad_x[off] = grad_x[off + hw] = grad_x[off + 2 * hw] = 0.f;
    return;
  }
  float r = 0.f, g = 0.f, bl = 0.f, dr = 0.f, dg = 0.f, db = 0.f;
  if (inside) {
    r = x[off];
    g = x[off + hw];
    bl = x[off + 2 * hw];
    dr = grad_out[off];
    dg = grad_out[off + hw];
    db = grad_out[off + 2 * hw];
  }
  const float fac = factor[b];
  float ro, go, bo;
  jpeg_forward<true>(L, r, g, bl, fac, 1, ro, go, bo);
  __syncthreads();  // every thread has read L.coef
  // / 255 and the clamp, then the transpose of YCbCr -> RGB
  dr = (ro > 0.f && ro < 255.f) ? dr / 255.f : 0.f;
  dg = (go > 0.f && go < 255.f) ? dg / 255.f : 0.f;
  db = (bo > 0.f && bo < 255.f) ? db / 255.f : 0.f;
  const int yb = (py >> 3) * 2 + (px >> 3);
  L.blk[yb][py & 7][px & 7] = (dr + dg) + db;
  L.pix[0][py][px] = -0.344136f * dg + 1.772f * db;
  L.pix[1][py][px] = 1.402f * dr + -0.714136f * dg;
  __syncthreads();
  chroma_pool(L, 1.f, 0.f);  // transpose of the 2x2 repeat
  __syncthreads();
  dct2(L, L.blk, L.coef);  // transpose of the inverse DCT
  for (int i = threadIdx.x; i < 384; i += 256) {
    const int bk = i >> 6, u = (i >> 3) & 7, v = i & 7;
    const float t = quant_table(bk, u, v) * fac, d = L.dq[bk][u][v];
    L.blk[bk][u][v] = (L.coef[bk][u][v] * t) * (3.f * (d * d)) / t;  // dequantise, rounding' = 3 (q - r)^2, quantise
  }
  __syncthreads();
  idct2(L, L.blk, L.coef, 0.f);  // transpose of the DCT
  const float ay = L.coef[yb][py & 7][px & 7];
  const float acb = 0.25f * L.coef[4][py >> 1][px >> 1], acr = 0.25f * L.coef[5][py >> 1][px >> 1];  // transpose of the 2x2 mean
  if (!in_buf) return;
  grad_x[off] = inside ? ((0.299f * ay + -0.168736f * acb) + 0.5f * acr) * 255.f : 0.f;
  grad_x[off + hw] = inside ? ((0.587f * ay + -0.331264f * acb) + -0.418688f * acr) * 255.f : 0.f;
  grad_x[off + 2 * hw] = inside ? ((0.114f * ay + 0.5f * acb) + -0.081312f * acr) * 255.f : 0.f;
}

bool plane_shape_ok(int B, int C, int H, int W) {
  return B > 0 && C > 0 && H > 0 && W > 0 && (long long)B * C <= 65535 && (long long)H * W < (1ll << 31) &&
         (long long)B * C * H * W < (1ll << 40);
}

}  // namespace

extern "C" int sr_filter2d_f32(const float* x, const float* kernels, float* out, int B, int C, int H, int W, int k, int kernel_batch,
                               void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && kernels && out, "sr_filter2d_f32: null pointer");
  SR_CHECK_ARG(plane_shape_ok(B, C, H, W), "sr_filter2d_f32: bad shape [%d, %d, %d, %d] (B * C at most 65535)", B, C, H, W);
  SR_CHECK_ARG(k >= 1 && k <= kFMaxK && (k & 1), "sr_filter2d_f32: kernel size %d is not supported: odd, 1..%d", k, kFMaxK);
  SR_CHECK_ARG(H > k / 2 && W > k / 2, "sr_filter2d_f32: a %dx%d image is too small to reflect by %d", H, W, k / 2);
  SR_CHECK_ARG(kernel_batch == 1 || kernel_batch == B, "sr_filter2d_f32: kernel_batch %d is neither 1 nor B = %d", kernel_batch, B);
  SR_CHECK_ARG(x != out, "sr_filter2d_f32: out must not be x");
  const bool prof = sr::prof_on();
  const double px = (double)B * C * H * W;
  if (prof) prof_rec(stream, 141, C, B, H, W, 2.0 * k * k * px, 8.0 * px);
  hipLaunchKernelGGL(filter2d_kernel, dim3(sr::cdiv(W, kFTileW), sr::cdiv(H, kFTileH), B * C), dim3(256), 0, stream, x, kernels, out,
                     C, H, W, k, kernel_batch);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_filter2d_f32");
  return SR_OK;
}

extern "C" int sr_resize_bilinear_f32(const float* src, const int32_t* src_sizes, float* dst, const int32_t* dst_sizes, int B, int C,
                                      int Hs, int Ws, int Hd, int Wd, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(src && dst, "sr_resize_bilinear_f32: null pointer");
  SR_CHECK_ARG(plane_shape_ok(B, C, Hs, Ws) && plane_shape_ok(B, C, Hd, Wd),
               "sr_resize_bilinear_f32: bad shape [%d, %d] %dx%d -> %dx%d (B * C at most 65535)", B, C, Hs, Ws, Hd, Wd);
  SR_CHECK_ARG(src != dst, "sr_resize_bilinear_f32: dst must not be src");
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 142, C, B, Hd, Wd, 8.0 * B * C * Hd * Wd, 4.0 * B * C * ((double)Hs * Ws + (double)Hd * Wd));
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3(sr::cdiv(Wd, 64), sr::cdiv(Hd, 4), B * C), dim3(256), 0, stream, src, src_sizes,
                     dst, dst_sizes, C, Hs, Ws, Hd, Wd);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_resize_bilinear_f32");
  return SR_OK;
}

extern "C" int sr_add_gaussian_noise_f32(const float* x, const float* noise, const float* noise_gray, const float* sigma,
                                         const float* gray, float* out, int B, int C, int H, int W, int clip, int rounds,
                                         void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && noise && sigma && out, "sr_add_gaussian_noise_f32: null pointer");
  SR_CHECK_ARG(!gray || noise_gray, "sr_add_gaussian_noise_f32: null pointer: gray needs noise_gray");
  SR_CHECK_ARG(plane_shape_ok(B, C, H, W) && B <= 65535 && C <= 65535,
               "sr_add_gaussian_noise_f32: bad shape [%d, %d, %d, %d] (B * C at most 65535)", B, C, H, W);
  const long long hw = (long long)H * W;
  const bool v4 = hw % 4 == 0 && sr::aligned16(x) && sr::aligned16(noise) && sr::aligned16(out) && (!gray || sr::aligned16(noise_gray));
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 143, C, B, H, W, 4.0 * B * C * hw, 12.0 * B * C * hw);
  const dim3 grid((unsigned)((hw + (v4 ? 1023 : 255)) / (v4 ? 1024 : 256)), C, B);
  if (v4)
    hipLaunchKernelGGL(gaussian_noise_kernel<4>, grid, dim3(256), 0, stream, x, noise, noise_gray, sigma, gray, out, C, hw, clip, rounds);
  else
    hipLaunchKernelGGL(gaussian_noise_kernel<1>, grid, dim3(256), 0, stream, x, noise, noise_gray, sigma, gray, out, C, hw, clip, rounds);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_add_gaussian_noise_f32");
  return SR_OK;
}

extern "C" int sr_diffjpeg_f32(const float* x, const int32_t* sizes, const float* factor, float* out, int B, int H, int W,
                               int differentiable, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && factor && out, "sr_diffjpeg_f32: null pointer");
  SR_CHECK_ARG(plane_shape_ok(B, 3, H, W) && sr::cdiv(H, 16) <= 65535, "sr_diffjpeg_f32: bad shape [%d, 3, %d, %d]", B, H, W);
  const bool prof = sr::prof_on();
  const double px = (double)B * H * W;
  if (prof) prof_rec(stream, 144, 3, B, H, W, 150.0 * px, 24.0 * px);
  hipLaunchKernelGGL(diffjpeg_kernel, dim3(sr::cdiv(W, 16), sr::cdiv(H, 16), B), dim3(256), 0, stream, x, sizes, factor, out, H, W,
                     differentiable ? 1 : 0);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_diffjpeg_f32");
  return SR_OK;
}

extern "C" int sr_diffjpeg_bwd_f32(const float* x, const int32_t* sizes, const float* factor, const float* grad_out, float* grad_x,
                                   int B, int H, int W, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && factor && grad_out && grad_x, "sr_diffjpeg_bwd_f32: null pointer");
  SR_CHECK_ARG(plane_shape_ok(B, 3, H, W) && sr::cdiv(H, 16) <= 65535, "sr_diffjpeg_bwd_f32: bad shape [%d, 3, %d, %d]", B, H, W);
  SR_CHECK_ARG(x != grad_x, "sr_diffjpeg_bwd_f32: grad_x must not be x");
  const bool prof = sr::prof_on();
  const double px = (double)B * H * W;
  if (prof) prof_rec(stream, 145, 3, B, H, W, 300.0 * px, 36.0 * px);
  hipLaunchKernelGGL(diffjpeg_bwd_kernel, dim3(sr::cdiv(W, 16), sr::cdiv(H, 16), B), dim3(256), 0, stream, x, sizes, factor, grad_out,
                     grad_x, H, W);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_diffjpeg_bwd_f32");
  return SR_OK;
}

extern "C" int sr_degrade_finish_f32(const float* x, const float* jitter, const float* gray, float* out, int B, int H, int W,
                                     const float* mean3, const float* std3, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && out, "sr_degrade_finish_f32: null pointer");
  SR_CHECK_ARG(plane_shape_ok(B, 3, H, W), "sr_degrade_finish_f32: bad shape [%d, 3, %d, %d]", B, H, W);
  FinishParams p = {};
  p.x = x;
  p.jitter = jitter;
  p.gray = gray;
  p.out = out;
  p.hw = (long long)H * W;
  p.normalise = (mean3 || std3) ? 1 : 0;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean3 ? mean3[c] : 0.f;
    p.stdv[c] = std3 ? std3[c] : 1.f;
  }
  const bool v4 = p.hw % 4 == 0 && sr::aligned16(x) && sr::aligned16(out);
  const bool prof = sr::prof_on();
  if (prof) prof_rec(stream, 146, 3, B, H, W, 12.0 * B * p.hw, 24.0 * B * p.hw);
  const dim3 grid((unsigned)((p.hw + (v4 ? 1023 : 255)) / (v4 ? 1024 : 256)), 1, B);
  if (v4)
    hipLaunchKernelGGL(degrade_finish_kernel<4>, grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(degrade_finish_kernel<1>, grid, dim3(256), 0, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("sr_degrade_finish_f32");
  return SR_OK;
}
