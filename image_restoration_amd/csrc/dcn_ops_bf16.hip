// Modulated deformable convolution (DCNv2) on v_mfma_f32_32x32x16_bf16 for gfx950 (include/sr_hip_edvr_bf16.h): forward only,
// the deformable conv of EDVR's bf16 inference forward.
//
// Structure of dcn_ops.hip's dcn_fwd_f32_kernel: a sampler writes the LDS column image [9 taps][rows][32][32 B] and the MFMA
// loop reads it like a halo-free tile.  Arithmetic of conv_bf16.hip's conv_bf16_kernel: a chunk is one CB16 block (16 channels),
// one MFMA per tap and (cout tile, row) consumes it; the weight image is sr_conv3x3_pack_bf16's mode-0 image, staged by LDS-DMA
// with the half-swap swizzle on the source address; accumulators, bias and LeakyReLU are fp32.
//
// Sampler.  A thread owns one (tile pixel, half) for the whole launch: half = 8 channels = 16 bytes of the block, its deformable
// group g = (16 cb + 8 half) / cpg.  Per chunk it runs the 9 taps.  The position, the `inside` test, the corner validity, the two
// fractions and the mask value (the sigmoid for logits) depend on (g, tap, pixel) only: they are kept in registers and computed
// again only when the chunk's group differs from the previous chunk's (cpg 8 and 16: every chunk; cpg 32: every second ...).
// Per item: up to four 16-byte corner loads, each checked against the image and nothing against the tile; the fp32 bilinear
// value w1 v1 + w2 v2 + w3 v3 + w4 v4 (left to right, -ffp-contract=off) times the mask; one round-to-nearest-even; one
// ds_write_b128 at ((tap * TH + row) * 32 + col) * 32 + (half ^ bit 3 of col) * 16, the address the MFMA loop's B operand of lane
// (pixel col, half) reads.
//
// LDS banks (the guide's rule: every ds_write has bank (a / 4) mod 32; a ds_write_b128 is served in 8 groups of 8 contiguous
// lanes): lanes 8 k .. 8 k + 7 of the sampler are the two halves of the 4 consecutive pixels 4 k' .. 4 k' + 3 of one tap row, and
// bit 3 of col is the same for the four, so the group writes 128 contiguous bytes: each of the 32 banks once.  The reads are
// conv_bf16.hip's (conflict-free by the half swap: lanes 8 apart fall on different 16-byte slots).
//
// LDS: column image 9 * 4 * 1 KiB = 36 KiB, single-buffered, + two weight units of 9 * COT KiB: 54 KiB (COT 1) / 72 KiB (COT 2)
// of 160 KiB, so two workgroups fit a CU at either COT and the sampler of one overlaps the MFMA loop of the other (the finding of
// the fp32 kernel: with one workgroup per CU the single-buffered column image serialises sampler and MFMA).  An 8-row tile
// (72 + 36 KiB) would leave one workgroup per CU and is not built.
#include <algorithm>

#include "cb16_tile.h"
#include "../../include/sr_hip_edvr_bf16.h"

using namespace cb16;

namespace {

struct DeformParams {
  const char* x;      // CB16 bf16
  const float* off;   // fp32 NCHW planes
  const float* msk;
  const char* w;      // bf16 image [group][cin/16][tap][32*COT][16]
  const float* bias;  // fp32 [cout pad 32] or null
  char* out;          // CB16 bf16
  long long x_nb, out_nb;  // image strides in bytes
  long long off_ns, msk_ns;  // in floats
  int cin_blocks, cout_blocks, cpg;
  int H, W;
  int tiles_x, tiles_y;
  int logit;
  float slope;
};

// One sampling position (the reference's dmcn_im2col_bilinear and the `inside` test of its caller): byte offset of the top-left
// corner inside a block plane, the two fractions, the mask value and which corners lie in the image (bits 0..3; 0 = outside).
struct Tap {
  int corner;
  unsigned valid;
  float lh, lw, m;
};

__device__ __forceinline__ Tap tap_at(float h_im, float w_im, float m, int H, int W) {
  Tap t;
  const bool inside = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  if (!inside) h_im = w_im = 0.f;  // also NaN and huge offsets: nothing below is used
  const float fh = floorf(h_im), fw = floorf(w_im);
  const int hl = (int)fh, wl = (int)fw;
  t.lh = h_im - fh;
  t.lw = w_im - fw;
  t.m = m;
  const bool top = hl >= 0, bot = hl + 1 <= H - 1, l = wl >= 0, r = wl + 1 <= W - 1;
  t.valid = inside ? ((top && l) ? 1u : 0u) | ((top && r) ? 2u : 0u) | ((bot && l) ? 4u : 0u) | ((bot && r) ? 8u : 0u) : 0u;
  t.corner = (hl * W + wl) * 32;
  return t;
}

// One 32-column x 4-row x (32*COT)-cout tile per workgroup of 4 waves.
template <int COT>
__global__ __launch_bounds__(256, 2) void deform16_fwd_kernel(const DeformParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = 4, TH = 4, NPIX = TH * 32;
  constexpr int CBYTES = 9 * NPIX * 32;  // column image
  constexpr int NWU = 9 * COT, WBYTES = NWU * 1024;
  constexpr int NWR = (NWU + NW - 1) / NW;
  static_assert(9 * NPIX * 2 == 9 * 256, "one sampler item per thread and tap");

  int t;
  {  // XCD-aware tile order (conv_bf16.hip)
    const int nwg = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  }
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int n = t / p.tiles_y;
  const int cog = blockIdx.y;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int x0 = tx * 32, y0 = ty * TH;
  const long long HW = (long long)p.H * p.W;
  const char* x_n = p.x + (long long)n * p.x_nb;
  const float* off_n = p.off + (long long)n * p.off_ns;
  const float* msk_n = p.msk + (long long)n * p.msk_ns;
  const char* wg = p.w + (size_t)cog * p.cin_blocks * WBYTES;

  const __amdgpu_buffer_rsrc_t w_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)wg, 0, (unsigned)((long long)p.cin_blocks * WBYTES), 0x00020000);
  const unsigned wvo = (lane ^ ((lane >> 4) & 1)) * 16;  // unit (cout i, half) <- half ^ bit3(i)
  char* cols = smem;
  auto stage_w = [&](int buf, int cb) {
    char* ws = smem + CBYTES + buf * WBYTES;
    const unsigned wso = (unsigned)cb * (unsigned)WBYTES;
#pragma unroll
    for (int r = 0; r < NWR; ++r) {
      const int u = r * NW + wave;  // unit = tap * COT + cout sub-tile
      if (u < NWU) sr::blds16(w_rs, wvo, wso + (unsigned)u * 1024u, ws + u * 1024);
    }
  };

  // the sampler's pixel: the two halves of a pixel are neighbouring lanes
  const int shalf = tid & 1, spix = tid >> 1;
  const int srow = spix >> 5, scol = spix & 31;
  const int sy = y0 + srow, sx = x0 + scol;
  const bool s_in = sy < p.H && sx < p.W;
  const long long s_pixoff = (long long)sy * p.W + sx;
  char* s_dst = cols + (srow * 32 + scol) * 32 + ((shalf ^ ((scol >> 3) & 1)) * 16);
  Tap taps[9];
  int cur_g = -1;

  auto sample = [&](int cb) {
    const int g = (cb * 16 + shalf * 8) / p.cpg;
    if (s_in && g != cur_g) {
      cur_g = g;
      const float* op = off_n + (long long)(18 * g) * HW + s_pixoff;
      const float* mp = msk_n + (long long)(9 * g) * HW + s_pixoff;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float oh = op[(2 * tap) * HW], ow = op[(2 * tap + 1) * HW];
        const float mv = mp[tap * HW];
        const float m = p.logit ? sigmoidf_(mv) : mv;
        const int ti = tap / 3, tj = tap - 3 * ti;
        taps[tap] = tap_at((float)(sy - 1 + ti) + oh, (float)(sx - 1 + tj) + ow, m, p.H, p.W);
      }
    }
    const char* xc = x_n + ((long long)cb * HW * 16 + shalf * 8) * 2;
    const long long down = (long long)p.W * 32;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      u32x4 o = {0u, 0u, 0u, 0u};
      if (s_in) {
        const Tap& b = taps[tap];
        const u32x4 z = {0u, 0u, 0u, 0u};
        const char* q = xc + b.corner;
        const u32x4 a1 = (b.valid & 1u) ? *(const u32x4*)q : z;
        const u32x4 a2 = (b.valid & 2u) ? *(const u32x4*)(q + 32) : z;
        const u32x4 a3 = (b.valid & 4u) ? *(const u32x4*)(q + down) : z;
        const u32x4 a4 = (b.valid & 8u) ? *(const u32x4*)(q + down + 32) : z;
        const float hh = 1.f - b.lh, hw = 1.f - b.lw;
        const float w1 = hh * hw, w2 = hh * b.lw, w3 = b.lh * hw, w4 = b.lh * b.lw;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (w1 * bf_at(a1, e) + w2 * bf_at(a2, e) + w3 * bf_at(a3, e) + w4 * bf_at(a4, e)) * b.m;
        o = pack8(v);
      }
      *(u32x4*)(s_dst + tap * (TH * 1024)) = o;
    }
  };

  f32x16 acc[COT][1];
#pragma unroll
  for (int a = 0; a < COT; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[a][0][e] = 0.f;

  const int xlane = (wave * 32 + j) * 32 + ((h ^ ((j >> 3) & 1)) * 16);
  const int wlane = j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  auto compute = [&](int buf) {
    const char* xb = cols + xlane;
    const char* ws = smem + CBYTES + buf * WBYTES + wlane;
    // taps in conv_bf16_kernel's order (column offset outer, row offset inner): with zero offsets and unit mask the accumulators
    // are then that kernel's bit for bit
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int tap = dy * 3 + dx;
        const bf16x8 b = *(const bf16x8*)(xb + tap * (TH * 1024));
#pragma unroll
        for (int c = 0; c < COT; ++c) {
          const bf16x8 a = *(const bf16x8*)(ws + (tap * COT + c) * 1024);
          acc[c][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[c][0], 0, 0, 0);
        }
      }
  };

  const int nchunk = p.cin_blocks;
  stage_w(0, 0);
  for (int c = 0; c < nchunk; ++c) {
    sample(c);
    __syncthreads();  // the column image of chunk c is written and its weight unit has arrived
    if (c + 1 < nchunk) stage_w((c + 1) & 1, c + 1);
    compute(c & 1);
    __syncthreads();
  }

  const int x = x0 + j, y = y0 + wave;
  const long long pix[1] = {(x < p.W && y < p.H) ? (long long)y * p.W + x : -1ll};
  epilogue<COT, 1>(acc, p.bias, p.slope, p.out + (long long)n * p.out_nb, HW, pix, cog, p.cout_blocks, h);
}

constexpr int deform_lds_bytes(int cot) { return 9 * 4 * 32 * 32 + 2 * 9 * cot * 1024; }

int check_desc(const sr_dcn_bf16_desc* d, const char* who) {
  SR_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  SR_CHECK_ARG(d->ksize == 3 && d->stride == 1 && d->padding == 1 && d->dilation == 1 && d->groups == 1,
               "%s: kernel %d stride %d padding %d dilation %d groups %d not supported (3x3, stride 1, padding 1, dilation 1, groups 1 "
               "only)",
               who, d->ksize, d->stride, d->padding, d->dilation, d->groups);
  SR_CHECK_ARG(d->x && d->offset && d->mask && d->wpacked && d->out, "%s: null x / offset / mask / wpacked / out", who);
  SR_CHECK_ARG(d->n > 0 && d->cin > 0 && d->cout > 0 && d->h > 0 && d->w > 0 && d->deformable_groups > 0, "%s: bad shape", who);
  SR_CHECK_ARG(d->cin % 16 == 0, "%s: cin %d must be a multiple of 16 (CB16)", who, d->cin);
  SR_CHECK_ARG(d->cin % d->deformable_groups == 0 && (d->cin / d->deformable_groups) % 8 == 0,
               "%s: cin %d / deformable_groups %d must be a multiple of 8 (a 16-byte half of a CB16 block never straddles two groups)",
               who, d->cin, d->deformable_groups);
  SR_CHECK_ARG(aligned16({d->x, d->wpacked, d->bpacked, d->out}) && ((uintptr_t)d->offset | (uintptr_t)d->mask) % 4 == 0 &&
                   (d->x_img_stride | d->out_img_stride) % 8 == 0,
               "%s: x / wpacked / bpacked / out must be 16-byte aligned (image strides multiples of 8), offset / mask 4-byte aligned",
               who);
  const long long hw = (long long)d->h * d->w, cob = (d->cout + 15) / 16;
  SR_CHECK_ARG(d->x_img_stride >= hw * d->cin && d->out_img_stride >= hw * 16 * cob &&
                   d->offset_img_stride >= hw * 18 * d->deformable_groups && d->mask_img_stride >= hw * 9 * d->deformable_groups,
               "%s: an image stride is smaller than the image", who);
  SR_CHECK_ARG(hw * 32 * std::max<long long>(d->cin / 16, cob) < (1ll << 31), "%s: image too large for 32-bit plane offsets", who);
  return SR_OK;
}

template <int COT>
int deform_launch(const DeformParams& p, int groups, const sr_dcn_bf16_desc* d, hipStream_t stream) {
  constexpr int lds = deform_lds_bytes(COT);
  static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
  auto kern = deform16_fwd_kernel<COT>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, lds)) return rc;
  const bool prof = sr::prof_on();
  if (prof) {
    const double px = (double)d->n * d->h * d->w;
    sr::prof_rec(stream, 124, d->cin, d->cout, d->n, d->h, d->w, 2.0 * 9 * d->cin * d->cout * px,
             px * (2.0 * (d->cin + d->cout) + 4.0 * 27 * d->deformable_groups));
  }
  hipLaunchKernelGGL(kern, dim3(p.tiles_x * p.tiles_y * d->n, groups), dim3(256), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("dcn_fwd_bf16 launch");
  return SR_OK;
}

}  // namespace

extern "C" size_t sr_dcn_bf16_lds_bytes(int cout, int n, int h, int w, int* cot, int* rows) {
  if (cout <= 0 || n <= 0 || h <= 0 || w <= 0) return 0;
  const int c = sr::group_couts(cout) / 32;
  if (cot) *cot = c;
  if (rows) *rows = 4;
  return (size_t)deform_lds_bytes(c);
}

extern "C" int sr_dcn_fwd_bf16(const sr_dcn_bf16_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_desc(d, "sr_dcn_fwd_bf16")) return rc;
  DeformParams p = {};
  p.x = (const char*)d->x;
  p.off = d->offset;
  p.msk = d->mask;
  p.w = (const char*)d->wpacked;
  p.bias = d->bpacked;
  p.out = (char*)d->out;
  p.x_nb = d->x_img_stride * 2;
  p.out_nb = d->out_img_stride * 2;
  p.off_ns = d->offset_img_stride;
  p.msk_ns = d->mask_img_stride;
  p.cin_blocks = d->cin / 16;
  p.cout_blocks = (d->cout + 15) / 16;
  p.cpg = d->cin / d->deformable_groups;
  p.H = d->h;
  p.W = d->w;
  p.tiles_x = sr::cdiv(d->w, 32);
  p.tiles_y = sr::cdiv(d->h, 4);
  p.logit = d->mask_is_logit;
  p.slope = d->act_slope;
  SR_CHECK_ARG((long long)p.tiles_x * p.tiles_y * d->n < (1ll << 31), "sr_dcn_fwd_bf16: grid too large");
  const int gc = sr::group_couts(d->cout);
  const int groups = ((d->cout + 31) / 32 * 32) / gc;
  return gc == 64 ? deform_launch<2>(p, groups, d, stream) : deform_launch<1>(p, groups, d, stream);
}
