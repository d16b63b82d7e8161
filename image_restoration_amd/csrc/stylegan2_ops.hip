// The `upfirdn2d` and `fused_act` extensions of the reference (basicsr/ops/upfirdn2d, basicsr/ops/fused_act) on gfx950
// (include/sr_hip_stylegan2.h).  Both are memory-bound: the aim is one read and one write per element.
//
// upfirdn2d.  A workgroup of 4 waves writes a tile of 64 columns x TH rows of one plane.  It first stages the source window of
// the tile, halo included and zero-filled outside the image, in LDS: source rows / columns [w0, w0 + W) with
// w0 = ceil((o0 * down - pad0) / up) and W = ((T - 1) * down + k - 1) / up + 1 (T = 64 or TH): every sample any tap of the tile
// meets.  The zero-inserted, padded tensor never exists.  Then it works polyphase: output o meets real samples only at the taps
// j = j0 + t * up with j0 = (-(o * down - pad0)) mod up, source index (o * down - pad0 + j) / up, filter index k - 1 - j.  The taps
// are taken in the order ky ascending, then kx ascending (j descending), one fmaf each, so an output is the same bits wherever
// its tile lies and whichever instance computes it.
//
// Tile and banks.  Lane = output column, so a wave stores 256 contiguous bytes of an output row and reads the window with
// ds_read_b32, which is served in two groups of 32 lanes over 32 banks (bank = dword address mod 32).  Per tap the 32 lanes of a
// group read
//   up >= down  source columns that advance by down / up <= 1 per lane: at most 32 consecutive dwords, equal ones broadcast: no
//               conflict (instances 1 and 2);
//   up 1, down d > 1   columns d apart, a d-way conflict in a plain image.  The window is therefore staged as d phase planes per
//               row, [row][phase = col mod d][col / d]: tap j of lane l reads plane j mod d at l + j / d, 32 consecutive dwords
//               again (instance 3 and the generic one).  The staging writes put the lanes of a group on d runs of 32 / d
//               consecutive banks: at worst 2-way at d = 2, which a ds_write_b32 hides behind its own data transfer.
// What is left to the generic instance alone is up > 1 with down > up (2 / 3 and the like): up to ceil(down / up)-way.
// 16-byte LDS reads would need 4 outputs per lane and 16-byte aligned output rows, which an arbitrary out_w does not give; with
// one row of 4 taps read once for the 8 output rows of a lane (below) the kernel issues 5.5 (instance 1), 4 (instance 2) and 9
// (instance 3) ds_read_b32 per output against 128 B/clk per CU, below what the 8 bytes per output cost in HBM time.
// The up-1 instances keep 8 output rows per lane in registers and walk the window rows once: each row's 4 values are read once
// and used by every output row they belong to.  TH = 32 (4 waves x 8 rows); LDS per workgroup 10.4 KiB (instance 1), 3.4 KiB
// (2), 34.5 KiB (3: 4 workgroups per CU).  The generic instance takes TH from the 63 KiB budget (sr_upfirdn2d_instance).
// A tile's time is the latency of its staging loads, not their bytes: the fixed-size instances index the window flat and keep
// up to 12 loads per thread in flight before the first LDS write; the generic instance stages row by row.
//
// fused bias + LeakyReLU: one kernel for the forward, the forward with `ref` (the second derivative) and the backward, which is
// the forward of (g, no bias, ref = out) plus a fixed-order sum of what it writes: thread, wave tree, workgroup, then a second
// launch over the partials (the tree is stated in the header).  16-byte accesses where inner is a multiple of 4.
#include <stdint.h>

#include "sr_internal.h"
#include "../../include/sr_hip_stylegan2.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kTileW = 64;
constexpr int kFilterFloats = 256;            // LDS floats in front of the window: the filter, kh * kw <= 256
constexpr size_t kLdsBudget = 63 * 1024;

struct UfdParams {
  const float* x;
  float* out;
  const float* filter;
  long long x_ns, out_ns;
  int planes, in_h, in_w, out_h, out_w;
  int kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0;
  int tiles_x, tiles_y, th;
  int ww, wh;      // window columns / rows staged per tile
  int np, split;   // columns of one phase plane, phase planes per row (down_x when up_x = 1, else 1)
};

__host__ __device__ __forceinline__ int ceil_div_s(int a, int b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }
__device__ __forceinline__ int pos_mod(int a, int b) {
  const int r = a % b;
  return r < 0 ? r + b : r;
}

// UP, DOWN, K: both axes' factors and the square filter size, fixed at compile time; K = 0: everything from the parameters.
template <int UP, int DOWN, int K>
__global__ __launch_bounds__(256) void upfirdn2d_kernel(const UfdParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* fl = smem;
  float* win = smem + kFilterFloats;
  const int upx = K ? UP : p.up_x, upy = K ? UP : p.up_y;
  const int dnx = K ? DOWN : p.down_x, dny = K ? DOWN : p.down_y;
  const int kh = K ? K : p.kh, kw = K ? K : p.kw;
  const int split = K ? DOWN : p.split;
  const int np = p.np, pitch = split * np;

  int t = blockIdx.x;
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int m = t / p.tiles_y;
  const int img = m / p.planes, ch = m - img * p.planes;
  const float* src = p.x + (long long)img * p.x_ns + (long long)ch * p.in_h * p.in_w;
  float* dst = p.out + (long long)img * p.out_ns + (long long)ch * p.out_h * p.out_w;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ox0 = tx * kTileW, oy0 = ty * p.th;
  const int wx0 = ceil_div_s(ox0 * dnx - p.pad_x0, upx), wy0 = ceil_div_s(oy0 * dny - p.pad_y0, upy);

  if (tid < kh * kw) fl[tid] = p.filter[tid];
  if constexpr (K != 0) {
    // the window's size is known: element e = i * 256 + tid in row-major order, up to 12 loads in flight per thread before
    // the first LDS write (a tile's time is the latency of its staging loads, not their bytes)
    constexpr int WW = ((kTileW - 1) * DOWN + K - 1) / UP + 1, WH = (31 * DOWN + K - 1) / UP + 1;
    constexpr int NLD = (WH * WW + 255) / 256, B = 12;
#pragma unroll
    for (int i0 = 0; i0 < NLD; i0 += B) {
      float v[B];
#pragma unroll
      for (int i = 0; i < B; ++i) {
        const int e = (i0 + i) * 256 + tid;
        const int row = e / WW, col = e - row * WW;
        const int sy = wy0 + row, sx = wx0 + col;
        v[i] = 0.f;
        if (i0 + i < NLD && e < WH * WW && sy >= 0 && sy < p.in_h && sx >= 0 && sx < p.in_w) v[i] = src[(long long)sy * p.in_w + sx];
      }
#pragma unroll
      for (int i = 0; i < B; ++i) {
        const int e = (i0 + i) * 256 + tid;
        const int row = e / WW, col = e - row * WW;
        if (i0 + i < NLD && e < WH * WW) win[row * pitch + (col % DOWN) * np + col / DOWN] = v[i];
      }
    }
  } else {
    for (int row = wave; row < p.wh; row += 4) {
      const int sy = wy0 + row;
      const bool row_ok = sy >= 0 && sy < p.in_h;
      for (int col = lane; col < p.ww; col += 64) {
        const int sx = wx0 + col;
        float v = 0.f;
        if (row_ok && sx >= 0 && sx < p.in_w) v = src[(long long)sy * p.in_w + sx];
        const int pos = split == 1 ? col : (col % split) * np + col / split;
        win[row * pitch + pos] = v;
      }
    }
  }
  __syncthreads();

  if constexpr (K != 0 && UP == 1) {
    // 8 output rows of one column per lane; window row (w * 8 + r) * DOWN + jy holds tap jy of output row r of wave w
    constexpr int R = 8, WR = (R - 1) * DOWN + K;
    float f[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) f[i] = fl[i];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    const float* wl = win + wave * R * DOWN * pitch + lane;
#pragma unroll
    for (int wr = WR - 1; wr >= 0; --wr) {
      float v[K];
#pragma unroll
      for (int jx = 0; jx < K; ++jx) v[jx] = wl[wr * pitch + (jx % DOWN) * np + jx / DOWN];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int jy = wr - r * DOWN;
        if (jy < 0 || jy >= K) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) acc[r] = __builtin_fmaf(v[K - 1 - kx], f[(K - 1 - jy) * K + kx], acc[r]);
      }
    }
    const int ox = ox0 + lane;
    if (ox < p.out_w) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int oy = oy0 + wave * R + r;
        if (oy < p.out_h) dst[(long long)oy * p.out_w + ox] = acc[r];
      }
    }
  } else {
    // with the factors fixed and K a multiple of UP every output meets exactly K / UP taps per axis: the loops unroll
    constexpr bool kFixedTaps = K != 0 && K % (UP ? UP : 1) == 0;
    const int n_out = kTileW * (K ? 32 : p.th);
#pragma unroll 4
    for (int idx = tid; idx < n_out; idx += 256) {
      const int ox = ox0 + (idx & 63), oy = oy0 + (idx >> 6);
      if (ox >= p.out_w || oy >= p.out_h) continue;
      const int by = oy * dny - p.pad_y0, bx = ox * dnx - p.pad_x0;
      const int jy0 = pos_mod(-by, upy), jx0 = pos_mod(-bx, upx);
      const int nty = kFixedTaps ? K / (UP ? UP : 1) : (jy0 < kh ? (kh - 1 - jy0) / upy + 1 : 0);
      const int ntx = kFixedTaps ? K / (UP ? UP : 1) : (jx0 < kw ? (kw - 1 - jx0) / upx + 1 : 0);
      float acc = 0.f;
      for (int a = nty - 1; a >= 0; --a) {
        const int jy = jy0 + a * upy;
        const float* wrow = win + ((by + jy) / upy - wy0) * pitch;
        const float* frow = fl + (kh - 1 - jy) * kw;
        for (int b = ntx - 1; b >= 0; --b) {
          const int jx = jx0 + b * upx;
          const int col = (bx + jx) / upx - wx0;
          const int pos = split == 1 ? col : (col % split) * np + col / split;
          acc = __builtin_fmaf(wrow[pos], frow[kw - 1 - jx], acc);
        }
      }
      dst[(long long)oy * p.out_w + ox] = acc;
    }
  }
}

struct UfdPlan {
  int instance, th, ww, wh, np, split;
  size_t lds;
};

// The dispatch, shared by the launch and sr_upfirdn2d_instance.  false: filter size or factors not supported.
bool ufd_plan(int kh, int kw, int up_x, int up_y, int down_x, int down_y, UfdPlan* q) {
  if (kh < 1 || kh > 16 || kw < 1 || kw > 16) return false;
  if (up_x < 1 || up_x > 8 || up_y < 1 || up_y > 8 || down_x < 1 || down_x > 8 || down_y < 1 || down_y > 8) return false;
  q->instance = 0;
  if (kh == 4 && kw == 4 && up_x == up_y && down_x == down_y) {
    if (up_x == 1 && down_x == 1) q->instance = 1;
    if (up_x == 2 && down_x == 1) q->instance = 2;
    if (up_x == 1 && down_x == 2) q->instance = 3;
  }
  q->split = up_x == 1 ? down_x : 1;
  q->ww = ((kTileW - 1) * down_x + kw - 1) / up_x + 1;
  q->np = (q->ww + q->split - 1) / q->split;
  for (int th = 32;; th /= 2) {
    q->th = th;
    q->wh = ((th - 1) * down_y + kh - 1) / up_y + 1;
    q->lds = ((size_t)kFilterFloats + (size_t)q->wh * q->np * q->split) * sizeof(float);
    if (q->lds <= kLdsBudget || th == 1) break;
  }
  return q->lds <= kLdsBudget && (q->instance == 0 || q->th == 32);
}

template <int UP, int DOWN, int K>
int ufd_launch(const UfdParams& p, const UfdPlan& plan, long long blocks, int n, hipStream_t stream) {
  auto kern = upfirdn2d_kernel<UP, DOWN, K>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, (int)plan.lds)) return rc;
  const bool prof = sr::prof_on();
  if (prof) {
    const double po = (double)n * p.planes * p.out_h * p.out_w, pi = (double)n * p.planes * p.in_h * p.in_w;
    const double taps = (double)((p.kh + p.up_y - 1) / p.up_y) * ((p.kw + p.up_x - 1) / p.up_x);
    sr::prof_rec(stream, 131 + plan.instance, p.planes, p.planes, n, p.in_h, p.in_w, 2.0 * taps * po, 4.0 * (pi + po));
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), plan.lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("upfirdn2d_f32 launch");
  return SR_OK;
}

// ------------------------------------------------------------------------------------------------ fused bias + LeakyReLU
__device__ __forceinline__ float bias_act(float x, float b, bool has_bias, float s, bool has_ref, float slope, float scale) {
  float t = has_bias ? x + b : x;
  t = (has_ref ? s : t) > 0.f ? t : t * slope;
  return t * scale;
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

// One chunk of 1024 * V values of one (n, c) row per workgroup: value (u * 256 + tid) * V + e of the chunk, u = 0 .. 3.
template <int V, bool REDUCE>
__global__ __launch_bounds__(256) void fused_bias_act_kernel(const float* x, const float* __restrict__ bias,
                                                             const float* ref, float* out, float* __restrict__ partial, int c,
                                                             long long inner, unsigned chunks, float slope, float scale) {
  const unsigned row = blockIdx.x / chunks, k = blockIdx.x - row * chunks;
  const bool has_bias = bias != nullptr, has_ref = ref != nullptr;
  const float b = has_bias ? bias[row % (unsigned)c] : 0.f;
  const long long base = (long long)row * inner;
  const int tid = threadIdx.x;
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long i = ((long long)k * 1024 + u * 256 + tid) * V;
    if (i >= inner) continue;
    if constexpr (V == 4) {
      const f32x4 xv = *(const f32x4*)(x + base + i);
      f32x4 rv = {0.f, 0.f, 0.f, 0.f}, y;
      if (has_ref) rv = *(const f32x4*)(ref + base + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = bias_act(xv[e], b, has_bias, rv[e], has_ref, slope, scale);
      *(f32x4*)(out + base + i) = y;
      if (REDUCE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s += y[e];
      }
    } else {
      const float y = bias_act(x[base + i], b, has_bias, has_ref ? ref[base + i] : 0.f, has_ref, slope, scale);
      out[base + i] = y;
      if (REDUCE) s += y;
    }
  }
  if constexpr (REDUCE) {
    __shared__ float wsum[4];
    s = wave_sum(s);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  }
}

// One wave per channel over its n * chunks partials, partial[(i * c + ch) * chunks + k] in the order i, then k.
__global__ __launch_bounds__(256) void fused_bias_act_finish_kernel(const float* __restrict__ partial, float* __restrict__ gbias, int n,
                                                                    int c, unsigned chunks) {
  const int lane = threadIdx.x & 63;
  const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
  float s = 0.f;
  if (ch < c) {
    const unsigned total = (unsigned)n * chunks;
    for (unsigned q = lane; q < total; q += 64) {
      const unsigned i = q / chunks, k = q - i * chunks;
      s += partial[((long long)i * c + ch) * chunks + k];
    }
  }
  s = wave_sum(s);
  if (lane == 0 && ch < c) gbias[ch] = s;
}

bool act_vec4(long long inner, std::initializer_list<const void*> ptrs) {
  if (inner % 4) return false;
  for (const void* q : ptrs)
    if ((uintptr_t)q % 16) return false;
  return true;
}

bool aligned4(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if ((uintptr_t)q % 4) return false;
  return true;
}

// workgroups of one pass at V values per thread and step; 0 when the grid would not fit 31 bits
long long act_blocks(int n, int c, long long inner, int v, unsigned* chunks) {
  const long long per_row = (inner + 1024ll * v - 1) / (1024ll * v);
  if (per_row >= (1ll << 31) || (long long)n * c >= (1ll << 31)) return 0;
  const long long blocks = per_row * n * c;
  if (blocks >= (1ll << 31)) return 0;
  *chunks = (unsigned)per_row;
  return blocks;
}

}  // namespace

extern "C" int sr_upfirdn2d_instance(int kh, int kw, int up_x, int up_y, int down_x, int down_y, int* tile_h, size_t* lds_bytes) {
  UfdPlan plan;
  if (!ufd_plan(kh, kw, up_x, up_y, down_x, down_y, &plan)) return -1;
  if (tile_h) *tile_h = plan.th;
  if (lds_bytes) *lds_bytes = plan.lds;
  return plan.instance;
}

extern "C" int sr_upfirdn2d_f32(const float* x, int64_t x_img_stride, float* out, int64_t out_img_stride, const float* filter, int n,
                                int planes, int in_h, int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x,
                                int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && out && filter, "sr_upfirdn2d_f32: null x/out/filter");
  SR_CHECK_ARG(aligned4({x, out, filter}), "sr_upfirdn2d_f32: pointers must be 4-byte aligned");
  SR_CHECK_ARG(minor == 1, "sr_upfirdn2d_f32: minor=%d is not supported (only minor 1, NCHW planes, is built)", minor);
  SR_CHECK_ARG(n > 0 && planes > 0 && in_h > 0 && in_w > 0, "sr_upfirdn2d_f32: bad shape n=%d planes=%d in=%dx%d", n, planes, in_h, in_w);
  UfdPlan plan;
  SR_CHECK_ARG(ufd_plan(kh, kw, up_x, up_y, down_x, down_y, &plan),
               "sr_upfirdn2d_f32: filter %dx%d, up (%d, %d), down (%d, %d) is not supported (filter sides 1..16, factors 1..8)", kh, kw,
               up_x, up_y, down_x, down_y);
  const long long lim = 1ll << 30;
  const auto mag = [](int v) { return v < 0 ? -(long long)v : (long long)v; };
  SR_CHECK_ARG((long long)in_w * up_x + mag(pad_x0) + mag(pad_x1) + kw < lim && (long long)in_h * up_y + mag(pad_y0) + mag(pad_y1) + kh < lim,
               "sr_upfirdn2d_f32: too large for the 32-bit coordinates of the kernel (in * up + |pad0| + |pad1| + k must be below 2^30)");
  const long long span_w = (long long)in_w * up_x + pad_x0 + pad_x1 - kw, span_h = (long long)in_h * up_y + pad_y0 + pad_y1 - kh;
  SR_CHECK_ARG(span_w >= 0 && span_h >= 0, "sr_upfirdn2d_f32: the output size is not positive (in %dx%d, pads x (%d, %d) y (%d, %d))", in_h,
               in_w, pad_x0, pad_x1, pad_y0, pad_y1);
  const int out_w = (int)(span_w / down_x) + 1, out_h = (int)(span_h / down_y) + 1;
  SR_CHECK_ARG(x_img_stride >= (long long)planes * in_h * in_w && out_img_stride >= (long long)planes * out_h * out_w,
               "sr_upfirdn2d_f32: image stride smaller than the image");
  UfdParams p = {};
  p.x = x;
  p.out = out;
  p.filter = filter;
  p.x_ns = x_img_stride;
  p.out_ns = out_img_stride;
  p.planes = planes;
  p.in_h = in_h;
  p.in_w = in_w;
  p.out_h = out_h;
  p.out_w = out_w;
  p.kh = kh;
  p.kw = kw;
  p.up_x = up_x;
  p.up_y = up_y;
  p.down_x = down_x;
  p.down_y = down_y;
  p.pad_x0 = pad_x0;
  p.pad_y0 = pad_y0;
  p.th = plan.th;
  p.ww = plan.ww;
  p.wh = plan.wh;
  p.np = plan.np;
  p.split = plan.split;
  p.tiles_x = sr::cdiv(out_w, kTileW);
  p.tiles_y = sr::cdiv(out_h, plan.th);
  const long long blocks = (long long)p.tiles_x * p.tiles_y * n * planes;
  SR_CHECK_ARG((long long)n * planes < (1ll << 31) && blocks < (1ll << 31), "sr_upfirdn2d_f32: grid too large (%lld tiles)", blocks);
  switch (plan.instance) {
    case 1: return ufd_launch<1, 1, 4>(p, plan, blocks, n, stream);
    case 2: return ufd_launch<2, 1, 4>(p, plan, blocks, n, stream);
    case 3: return ufd_launch<1, 2, 4>(p, plan, blocks, n, stream);
    default: return ufd_launch<0, 0, 0>(p, plan, blocks, n, stream);
  }
}

extern "C" int sr_fused_bias_act_f32(const float* x, const float* bias, const float* ref, float* out, int n, int c, int64_t inner,
                                     float slope, float scale, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(x && out, "sr_fused_bias_act_f32: null x/out");
  SR_CHECK_ARG(aligned4({x, bias, ref, out}), "sr_fused_bias_act_f32: pointers must be 4-byte aligned");
  SR_CHECK_ARG(n > 0 && c > 0 && inner > 0, "sr_fused_bias_act_f32: bad shape n=%d c=%d inner=%lld", n, c, (long long)inner);
  const int v = act_vec4(inner, {x, ref, out}) ? 4 : 1;
  unsigned chunks = 0;
  const long long blocks = act_blocks(n, c, inner, v, &chunks);
  SR_CHECK_ARG(blocks > 0, "sr_fused_bias_act_f32: grid too large");
  const bool prof = sr::prof_on();
  const double total = (double)n * c * (double)inner;
  if (prof) sr::prof_rec(stream, 135, c, c, n, 1, (int)(inner < (1ll << 31) ? inner : 0), 3.0 * total, 4.0 * total * (ref ? 3 : 2));
  if (v == 4)
    hipLaunchKernelGGL((fused_bias_act_kernel<4, false>), dim3((unsigned)blocks), dim3(256), 0, stream, x, bias, ref, out, (float*)nullptr, c,
                       (long long)inner, chunks, slope, scale);
  else
    hipLaunchKernelGGL((fused_bias_act_kernel<1, false>), dim3((unsigned)blocks), dim3(256), 0, stream, x, bias, ref, out, (float*)nullptr, c,
                       (long long)inner, chunks, slope, scale);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("fused_bias_act launch");
  return SR_OK;
}

// partials of the scalar pass, the larger of the two
extern "C" size_t sr_fused_bias_act_workspace_bytes(int n, int c, int64_t inner) {
  unsigned chunks = 0;
  if (n <= 0 || c <= 0 || inner <= 0) return 0;
  const long long blocks = act_blocks(n, c, inner, 1, &chunks);
  return (size_t)blocks * sizeof(float);
}

extern "C" int sr_fused_bias_act_bwd_f32(const float* g, const float* out, float* gx, float* gbias, int n, int c, int64_t inner,
                                         float slope, float scale, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SR_CHECK_ARG(g && out && gx, "sr_fused_bias_act_bwd_f32: null g/out/gx");
  SR_CHECK_ARG(aligned4({g, out, gx, gbias, workspace}), "sr_fused_bias_act_bwd_f32: pointers must be 4-byte aligned");
  SR_CHECK_ARG(n > 0 && c > 0 && inner > 0, "sr_fused_bias_act_bwd_f32: bad shape n=%d c=%d inner=%lld", n, c, (long long)inner);
  const int v = act_vec4(inner, {g, out, gx}) ? 4 : 1;
  unsigned chunks = 0, chunks1 = 0;
  const long long blocks = act_blocks(n, c, inner, v, &chunks);
  SR_CHECK_ARG(blocks > 0 && act_blocks(n, c, inner, 1, &chunks1) > 0, "sr_fused_bias_act_bwd_f32: grid too large");
  if (gbias) {
    SR_CHECK_ARG(workspace != nullptr, "sr_fused_bias_act_bwd_f32: gbias needs a workspace");
    if (workspace_bytes < sr_fused_bias_act_workspace_bytes(n, c, inner)) {
      sr::set_error("sr_fused_bias_act_bwd_f32: workspace of %zu bytes, %zu needed", workspace_bytes,
                    sr_fused_bias_act_workspace_bytes(n, c, inner));
      return SR_ENOSPACE;
    }
  }
  float* partial = (float*)workspace;
  const bool prof = sr::prof_on();
  const double total = (double)n * c * (double)inner;
  if (prof) sr::prof_rec(stream, 136, c, c, n, 1, (int)(inner < (1ll << 31) ? inner : 0), 3.0 * total, 4.0 * total * 3);
#define SR_ACT_BWD(V, RED)                                                                                                          \
  hipLaunchKernelGGL((fused_bias_act_kernel<V, RED>), dim3((unsigned)blocks), dim3(256), 0, stream, g, (const float*)nullptr, out, gx, \
                     partial, c, (long long)inner, chunks, slope, scale)
  if (v == 4) {
    if (gbias) SR_ACT_BWD(4, true); else SR_ACT_BWD(4, false);
  } else {
    if (gbias) SR_ACT_BWD(1, true); else SR_ACT_BWD(1, false);
  }
#undef SR_ACT_BWD
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("fused_bias_act_bwd launch");
  if (!gbias) return SR_OK;
  if (prof) sr::prof_rec(stream, 137, c, c, n, 1, (int)chunks, (double)blocks, 4.0 * ((double)blocks + c));
  hipLaunchKernelGGL(fused_bias_act_finish_kernel, dim3((unsigned)sr::cdiv(c, 4)), dim3(256), 0, stream, (const float*)partial, gbias, n, c,
                     chunks);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("fused_bias_act_finish launch");
  return SR_OK;
}
