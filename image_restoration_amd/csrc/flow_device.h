// Device code shared by flow_ops.hip (include/sr_hip_flow.h), flow_bwd_ops.hip (include/sr_hip_flow_bwd.h) and tof_ops.hip
// (include/sr_hip_tof.h): the implicit-GEMM body of the 7x7 and 9x9 convolutions (conv_body: SpyNet's forward and data gradient,
// TOFlow's 9x9), the sampling position and corner rule of flow warping, and the pyramid level input of SpyNet and SPyNetTOF
// (level_input_body).  Everything is __device__ __forceinline__: each kernel that uses a body gets its own copy of the
// instructions, and what a kernel lacks is compiled out (if constexpr on the constants of its parameter struct), never tested
// at run time.  With conv_body taking its parameters by value the 7x7 kernels compile to the instructions they had when the body
// lived in flow_ops.hip, up to register numbering, the operand order of one multiply-add in the epilogue's address arithmetic and
// the placement of one s_nop (compared by disassembly); DESIGN section 40 has the comparison for the 9x9.
#pragma once
#include <math.h>

#include "sr_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace flowdev {

// ------------------------------------------------------------------------------------------- conv 7x7 and 9x9, one body
constexpr int x_row(int ks) { return 32 + ks - 1; }  // columns of the halo'd X tile
constexpr int kKS = 7, kXRow = x_row(kKS);

// Kernel arguments of the body below.  The static members tell it at compile time what a kernel has: KS taps (pad KS / 2), cout
// groups over blockIdx.y with the cout_blocks test and res1 (kGroups), the mask of the channels beyond cin in the last block
// (kCinMask).  They take no room in the kernarg.
struct C7Params {
  static constexpr int KS = 7;
  static constexpr bool kGroups = true, kCinMask = false;
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  const float* res1;
  long long in_ns, out_ns, res1_ns;
  int cin_blocks, cout_blocks, cout, H, W, tiles_x, tiles_y, relu;
};
struct C7MaskParams : C7Params {  // the data gradient: out *= (mask > 0), mask shaped like out
  const float* mask;
  long long mask_ns;
};
struct C9Params {  // TOFlow's 9x9 (tof_ops.hip): 64 couts in one group; cin = 21 leaves channels 21-23 of the last block unread
  static constexpr int KS = 9;
  static constexpr bool kGroups = false, kCinMask = true;
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  long long in_ns, out_ns;
  int cin, cin_blocks, H, W, tiles_x, tiles_y, relu;
};

__device__ __forceinline__ int xcd_tile(int nwg, int b) {  // XCD-aware tile order, as conv_f32_kernel
  const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// Per-lane byte offsets of the X pieces this wave stages (pad lanes: an offset beyond the descriptor, which reads as zero).
template <int NXR, int XPIX, int KS = kKS>
__device__ __forceinline__ void x_offsets(unsigned (&xvo)[NXR], int wave, int lane, int x0, int y0, int H, int W) {
#pragma unroll
  for (int r = 0; r < NXR; ++r) {
    const int q = (r * 4 + wave) * 64 + lane;
    const int pix = q >> 1, half = q & 1;
    const int row = pix / x_row(KS), col = pix - row * x_row(KS);
    const int gy = y0 - KS / 2 + row, gx = x0 - KS / 2 + col;
    const bool valid = pix < XPIX && gy >= 0 && gy < H && gx >= 0 && gx < W;
    // LDS bank swizzle, as conv_tile_f32: the 16-byte halves of tile column c are stored swapped when bit 3 of c is set
    const int hsw = half ^ ((col >> 3) & 1);
    xvo[r] = valid ? (unsigned)((gy * W + gx) * 8 + hsw * 4) * 4u : 0xfffffff0u;
  }
}

template <int PT>
constexpr int conv_tile_rows() {
  return 4 * PT;
}
template <int COT, int PT, int KS = kKS>
constexpr int conv_lds_bytes() {
  return 2 * (((((conv_tile_rows<PT>() + KS - 1) * x_row(KS) * 32 + 1023) / 1024) * 1024) + KS * COT * 1024);
}

// The workgroup's whole job: 256 threads, conv_lds_bytes<COT, PT, P::KS>() bytes of dynamic LDS at smem.  Output tile = (4 * PT
// rows) x 32 columns x (32 * COT couts); K = KS * KS * cin is walked in chunks of (one 8-channel block, one tap row).  MASK = false
// is a forward (P = C7Params, C9Params); MASK = true (P = C7MaskParams) zeroes an output element whose mask element is not
// positive, after everything else.
template <int COT, int PT, bool MASK, class P>
__device__ __forceinline__ void conv_body(const P p, char* smem) {
  constexpr int KS = P::KS, XROW = x_row(KS);
  constexpr int TH = conv_tile_rows<PT>(), XPIX = (TH + KS - 1) * XROW;
  constexpr int XBYTES = ((XPIX * 32 + 1023) / 1024) * 1024, NXU = XBYTES / 1024, NXR = (NXU + 3) / 4;
  constexpr int NWU = KS * COT, WBYTES = NWU * 1024, NWR = (NWU + 3) / 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  int t = xcd_tile(gridDim.x, blockIdx.x);
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y, n = t / p.tiles_y;
  int cog = 0;
  if constexpr (P::kGroups) cog = blockIdx.y;
  const int x0 = tx * 32, y0 = ty * TH;
  const int HW = p.H * p.W;
  const float* in_n = p.in + (long long)n * p.in_ns;
  const float* wg = p.w + (size_t)cog * p.cin_blocks * (KS * WBYTES / 4);

  unsigned xvo[NXR];
  x_offsets<NXR, XPIX, KS>(xvo, wave, lane, x0, y0, p.H, p.W);
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)in_n, 0, (unsigned)p.cin_blocks * (unsigned)HW * 32u, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)wg, 0, (unsigned)p.cin_blocks * (unsigned)(KS * WBYTES), 0x00020000);
  const unsigned wvo = (unsigned)(lane ^ ((lane >> 4) & 1)) * 16u;  // unit (cout i, half) <- half ^ bit3(i)
  char* const xs0 = smem;
  char* const ws0 = smem + 2 * XBYTES;
  auto stage_x = [&](int buf, int cb) {
    char* xs = xs0 + buf * XBYTES;
    const unsigned so = (unsigned)cb * (unsigned)HW * 32u;
#pragma unroll
    for (int r = 0; r < NXR; ++r) {
      const int u = r * 4 + wave;
      if (u < NXU) sr::blds16(x_rs, xvo[r], so, xs + u * 1024);
    }
  };
  auto stage_w = [&](int buf, int chunk) {  // chunk = cb * KS + tap row
    char* ws = ws0 + buf * WBYTES;
    const unsigned so = (unsigned)chunk * (unsigned)WBYTES;
#pragma unroll
    for (int r = 0; r < NWR; ++r) {
      const int u = r * 4 + wave;  // unit = tap column * COT + cout sub-tile
      if (u < NWU) sr::blds16(w_rs, wvo, so + (unsigned)u * 1024u, ws + u * 1024);
    }
  };

  f32x16 acc[COT][PT];
#pragma unroll
  for (int a = 0; a < COT; ++a)
#pragma unroll
    for (int b = 0; b < PT; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  int xlane[KS];  // byte offset of this lane's B operand at tap column dx (tap row 0, row group 0), swizzled half
#pragma unroll
  for (int dx = 0; dx < KS; ++dx) xlane[dx] = ((wave * PT) * XROW + j + dx) * 32 + ((h ^ (((j + dx) >> 3) & 1)) * 16);
  const int wlane = j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  // lim (kCinMask): how many of this lane's 4 channels of the block are real; the others are replaced by zero after the read
  auto compute = [&](int xbuf, int wbuf, int dy, int lim) {
    const char* xb = xs0 + xbuf * XBYTES + dy * (XROW * 32);
    const char* ws = ws0 + wbuf * WBYTES + wlane;
#pragma unroll
    for (int dx = 0; dx < KS; ++dx) {
      f32x4 a[COT], b[PT];
#pragma unroll
      for (int c = 0; c < COT; ++c) a[c] = *(const f32x4*)(ws + (dx * COT + c) * 1024);
#pragma unroll
      for (int r = 0; r < PT; ++r) {
        b[r] = *(const f32x4*)(xb + xlane[dx] + r * (XROW * 32));
        if constexpr (P::kCinMask) {
#pragma unroll
          for (int s = 1; s < 4; ++s) b[r][s] = s < lim ? b[r][s] : 0.f;
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int c = 0; c < COT; ++c)
#pragma unroll
          for (int r = 0; r < PT; ++r) acc[c][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][s], b[r][s], acc[c][r], 0, 0, 0);
    }
  };

  const int nchunk = p.cin_blocks * KS;
  stage_x(0, 0);
  stage_w(0, 0);
  __syncthreads();
  int cb = 0, dy = 0;
  for (int c = 0; c < nchunk; ++c) {
    if (c + 1 < nchunk) stage_w((c + 1) & 1, c + 1);
    if (dy == 0 && cb + 1 < p.cin_blocks) stage_x((cb + 1) & 1, cb + 1);  // that buffer was last read in block cb - 1
    int lim = 4;
    if constexpr (P::kCinMask) lim = p.cin - cb * 8 - h * 4;
    compute(cb & 1, c & 1, dy, lim);
    __syncthreads();  // drains the LDS-DMA issued above and frees the buffers just read
    if (++dy == KS) {
      dy = 0;
      ++cb;
    }
  }

  // ---- epilogue: bias, ReLU [, res1] [, mask]
  const int x = x0 + j;
#pragma unroll
  for (int r = 0; r < PT; ++r) {
    const int y = y0 + wave * PT + r;
    if (y >= p.H || x >= p.W) continue;
    const long long pixoff = (long long)y * p.W + x;
#pragma unroll
    for (int c = 0; c < COT; ++c) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ob = (cog * COT + c) * 4 + g;
        if constexpr (P::kGroups) {
          if (ob >= p.cout_blocks) continue;
        }
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[c][r][g * 4 + e];
        const long long off = ((long long)ob * HW + pixoff) * 8 + h * 4;
        v += *(const f32x4*)(p.bias + ob * 8 + h * 4);
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        if constexpr (P::kGroups) {
          if (p.res1) v += *(const f32x4*)(p.res1 + (long long)n * p.res1_ns + off);
        }
        if constexpr (MASK) {
          if (p.mask) {
            const f32x4 m = *(const f32x4*)(p.mask + (long long)n * p.mask_ns + off);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
          }
        }
        *(f32x4*)(p.out + (long long)n * p.out_ns + off) = v;
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------- flow warping
// The sampling position of output pixel (y, x); false: every corner lies outside the image (zeros padding), the result is 0.
// gx_on / gy_on: the axis passes a gradient to the flow (size > 1 and, under border, not clipped).
__device__ __forceinline__ bool warp_coord(float flx, float fly, int x, int y, int H, int W, int border, int& x0, int& y0,
                                           float& fx, float& fy, bool& gx_on, bool& gy_on) {
  float ix = W > 1 ? (float)x + flx : 0.f, iy = H > 1 ? (float)y + fly : 0.f;
  gx_on = W > 1;
  gy_on = H > 1;
  if (border) {
    const float mx = (float)(W - 1), my = (float)(H - 1);
    if (!(ix >= 0.f && ix <= mx)) gx_on = false;
    if (!(iy >= 0.f && iy <= my)) gy_on = false;
    ix = fminf(fmaxf(ix, 0.f), mx);
    iy = fminf(fmaxf(iy, 0.f), my);
  } else if (!(ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H)) {
    return false;
  }
  const float flx0 = floorf(ix), fly0 = floorf(iy);
  x0 = (int)flx0;
  y0 = (int)fly0;
  fx = ix - flx0;
  fy = iy - fly0;
  return true;
}

struct Corners {  // validity and plane offsets (pixels) of the four corners
  bool ok[4];
  int off[4];
};
__device__ __forceinline__ Corners corners(int x0, int y0, int H, int W) {
  Corners c;
  const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W, ya = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
  c.ok[0] = ya && xa;
  c.ok[1] = ya && xb;
  c.ok[2] = yb && xa;
  c.ok[3] = yb && xb;
  c.off[0] = y0 * W + x0;
  c.off[1] = c.off[0] + 1;
  c.off[2] = c.off[0] + W;
  c.off[3] = c.off[2] + 1;
  return c;
}
__device__ __forceinline__ float blend(double v00, double v01, double v10, double v11, float fx, float fy) {
  const double gx = fx, gy = fy;
  return (float)((1.0 - gy) * ((1.0 - gx) * v00 + gx * v01) + gy * ((1.0 - gx) * v10 + gx * v11));
}

// ------------------------------------------------------------------------------------------------------- SpyNet pieces
__device__ __forceinline__ void up_coord(int d, int dst_len, int src_len, int& i0, int& i1, double& f) {
  const double s = dst_len > 1 ? (double)d * (double)(src_len - 1) / (double)(dst_len - 1) : 0.0;
  i0 = min((int)s, src_len - 1);
  i1 = min(i0 + 1, src_len - 1);
  f = s - (double)i0;
}

// One thread of a pyramid level's input: [ref, warp(supp, up), up] of pixel blockIdx.x * 256 + threadIdx.x of image blockIdx.z as
// one CB8 block, and up (twice the coarser level's flow, resized x2 with align_corners) as another.  ``rimg`` / ``simg``: the three
// planes of this image's reference and of the frame that is warped; BORDER: the padding of the warp (1: SpyNet, 0: SPyNetTOF).
template <int BORDER>
__device__ __forceinline__ void level_input_body(const float* __restrict__ rimg, const float* __restrict__ simg,
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
  const bool any = warp_coord(ux, uy, px, py, H, W, BORDER, x0, y0, fx, fy, gx_on, gy_on);  // always true under border
  Corners k = {};
  if (any) k = corners(x0, y0, H, W);
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

struct Norm3 {  // per-channel mean and std of the RGB normalisation, passed by value
  float mean[3], stdv[3];
};

}  // namespace flowdev
