// Winograd F(2x2,3x3) convolution on fp32 MFMA for gfx950 (MI355X): the 3x3 / stride 1 / pad 1 convs of the fp32 INFERENCE forward
// of RRDBNet (RDB conv1-5, conv_body, conv_up1/2, conv_hr: rrdbnet_arch.py:32-39, :113-117) with 16 multiplies per (cin, cout) and
// 2x2 output patch instead of 36.
//
//   Y = A^T [ sum_cin (G g G^T) . (B^T d B) ] A      d = 4x4 input patch, g = 3x3 filter, Y = 2x2 output patch
//
// U = G g G^T comes pre-transformed from the weight packer (pack_net.hip, kind 3: float64, rounded once).  Per transform point
// the sum over cin is a GEMM  M_p[cout][patch] += U_p[cout][cin] * V_p[cin][patch]  on v_mfma_f32_32x32x2_f32, with the operand
// roles of conv_f32.hip (A = weights, B = activations): the 32x32 accumulator has the PATCH on the lane and 4 consecutive couts
// in 4 consecutive registers, so all 16 points of one (cout, patch) sit in ONE lane, in 16 different accumulators — the output
// transform is 24 per-lane adds and the epilogue's 16-byte CB8 stores are those of the direct kernel.
//
// One wave = 32 patches (one patch row, 64 pixel columns) x 32 couts x 8 points = 128 accumulator registers: the 16 points are split
// by transform row over TWO waves, "low" (rows r = 0, 1 of V = B^T d B: points 0-7) and "high" (r = 2, 3: points 8-15), so a wave
// fits in 256 registers and two waves share a SIMD: each covers the other's LDS reads, transform adds, barrier waits and epilogue.
// Workgroup = 2 NW waves = NW patch rows x 2 halves (waves 0..NW-1 low, NW..2NW-1 high: at NW = 4 the two halves of a patch row are
// the two waves of one SIMD): output tile (2 NW rows) x 64 columns x 32 couts; blockIdx.y = 32-cout group.
// K is walked in chunks of one 8-channel CB8 block, one barrier per chunk; U is double buffered, X triple buffered (the operand
// of chunk c + 1 is formed under the MFMAs of chunk c):
//   LDS X image  [2 NW + 2][66][8] floats   raw halo'd tile, staged like conv_tile_f32 (buffer-descriptor LDS-DMA through the
//                                           source map: zero padding = out-of-range offsets, nearest x2 upsample = src >> 1)
//   LDS U image  [16 points][32 couts][8]   contiguous in HBM
// Per chunk a lane (patch j, half h) reads the three raw rows its two transform rows need (d0 d1 d2 low, d1 d2 d3 high), four
// columns of channels 4h..4h+3 (12 ds_read_b128), forms its 8 values of V = B^T d B in registers and issues 8 points x 4 K=2
// steps = 32 MFMAs on its 8 U planes.  Behind the last chunk the column step of the output transform is per wave; the row step
// needs one transform row of the other half, exchanged once per tile through the then-dead U buffers (NW = 4: X buffers).  Low
// stores output row dy = 0 of its patch row, high dy = 1.  Residual 1 of the tile is brought into the X buffers by LDS-DMA under the
// MFMAs of the last chunk (NW = 2, 1; two chunks or more), so that the epilogue reads it from the LDS, not by dependent global loads.
//
// Patches are anchored at EVEN image coordinates, chunks ascend, the order inside a chunk and every expression tree are fixed and
// every variant (NW = 4, 2, 1) runs the same wave code: an output value depends on its image and its position only — not on tile
// shape, launch size or batch.  No inter-workgroup communication of any kind.
#include <stdlib.h>

#include <type_traits>

#include "sr_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

struct WinoParams {
  const float* in;
  const float* u;  // [cout / 32][cin_blocks][16][32][8]
  const float* bias;
  float* out;
  const float* res1;
  const float* res2;
  long long in_ns, out_ns, res1_ns, res2_ns;
  int cin_blocks, cout_blocks;
  int in_h, in_w;  // real source size
  int H, W;        // output size (= source size, or twice it through the nearest x2 source map)
  int tiles_x, tiles_y;
  int src_shift;
  int res_cb1;
  int res_stage;  // residual 1 through the LDS (sr_dev_set_wino_res_stage)
  float slope, alpha, beta1, beta2;
#ifdef SR_WINO_STAMP
  unsigned long long* stamps;  // diagnostic build only (tools/wino_phase.py): [workgroup][8] s_memtime values
#endif
};

// Phase stamps of the diagnostic build (`make stamp`: its own library, never the product's): one lane per workgroup writes the clock
// at entry, behind the first barrier, behind the last chunk's barrier, behind the exchange and behind its last store (0-4), and at
// the head of the last chunk (5).
#ifdef SR_WINO_STAMP
#define WINO_STAMP(k)                                                                                               \
  do {                                                                                                              \
    if (p.stamps && wave == 0 && lane == 0)                                                                         \
      p.stamps[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (k)] = __builtin_amdgcn_s_memtime();             \
  } while (0)
#else
#define WINO_STAMP(k) \
  do {                \
  } while (0)
#endif

constexpr int XROW = 66;  // 64 tile columns + halo

template <int NW>
constexpr int wino_x_bytes() {
  return (((2 * NW + 2) * XROW * 32 + NW * 1024 - 1) / (NW * 1024)) * (NW * 1024);  // whole 1 KiB pieces, a multiple of NW of them
}
template <int NW>
constexpr int wino_lds_bytes() {
  return 3 * wino_x_bytes<NW>() + 2 * 16 * 1024;
}

// One output tile as seen by one wave of half HF (0 = low: transform rows 0, 1; 1 = high: rows 2, 3); the body of
// conv_wino_f32_kernel (a __device__ function: the host pass does not see the target builtins).  Both halves pass the same barriers.
template <int NW, int HF>
__device__ __forceinline__ void conv_wino_tile_f32(const WinoParams p, char* smem, const int wave) {
  constexpr int NV = 2 * NW;  // waves of the workgroup
  constexpr int XPIX = (2 * NW + 2) * XROW;
  constexpr int XBYTES = wino_x_bytes<NW>();
  constexpr int NXU = (XPIX * 32 + 1023) / 1024, NWU = 16;  // 1 KiB pieces of one X chunk / one U chunk
  constexpr int NXR = (NXU + NV - 1) / NV, NWR = NWU / NV;  // per wave; the last X round is guarded (piece < NXU)
  // Behind the last chunk's barrier both U buffers are dead: at NW = 2, 1 the exchange of the output transform (8 KiB per wave) lives
  // there, and the X region holds residual 1 of the output tile (2 NW rows x 4 channel blocks x 2 KiB).  At NW = 4 the exchange does
  // not fit the U region: it stays in the X buffers and the residual stays a global load.
  constexpr bool RES_LDS = NW <= 2;
  constexpr int XCH = RES_LDS ? 3 * XBYTES : 0;  // byte offset of the exchange
  static_assert(RES_LDS ? NV * 8192 <= 2 * NWU * 1024 : NV * 8192 <= 3 * XBYTES,
                "the exchange of the output transform lives in the U buffers (NW = 2, 1) or in the X buffers (NW = 4)");
  static_assert(!RES_LDS || NW * 16384 <= 3 * XBYTES, "the staged residual tile lives in the X buffers");

  // XCD-aware tile order (as conv_f32_kernel): each XCD gets a contiguous run of tiles
  int t;
  {
    const int nwg = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  }
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int n = t / p.tiles_y;
  const int cog = blockIdx.y;

  const int lane = threadIdx.x & 63;
  WINO_STAMP(0);
  const int prow = wave - HF * NW;  // patch row of the tile
  const int j = lane & 31, h = lane >> 5;
  const int x0 = tx * 64, y0 = ty * (2 * NW);
  const int HWin = p.in_h * p.in_w;
  const float* in_n = p.in + (long long)n * p.in_ns;
  const float* ug = p.u + (size_t)cog * p.cin_blocks * (NWU * 256);

  // per-lane byte offsets (inside one channel-block plane) of the X pieces this wave moves; padding lanes carry an offset beyond
  // num_records and read zeros
  unsigned xvo[NXR];
#pragma unroll
  for (int r = 0; r < NXR; ++r) {
    const int u = r * NV + wave;
    const int q = u * 64 + lane;
    const int pix = q >> 1, half = q & 1;
    const int row = pix / XROW, col = pix - row * XROW;
    const int gy = y0 - 1 + row, gx = x0 - 1 + col;
    const bool valid = pix < XPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
    const int sy = gy >> p.src_shift, sx = gx >> p.src_shift;
    // LDS bank swizzle: the two 16-byte halves of tile column c are stored swapped when bit 3 of c is set (the readers' lanes
    // stride 64 B: without it lanes j and j + 4 meet in one bank slot)
    const int hsw = half ^ ((col >> 3) & 1);
    xvo[r] = valid ? (unsigned)((sy * p.in_w + sx) * 8 + hsw * 4) * 4u : 0xfffffff0u;
  }
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)in_n, 0, (unsigned)((long long)p.cin_blocks * HWin * 32), 0x00020000);
  const __amdgpu_buffer_rsrc_t u_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)ug, 0, (unsigned)((long long)p.cin_blocks * NWU * 1024), 0x00020000);
  const unsigned uvo = (lane ^ ((lane >> 4) & 1)) * 16;  // unit (cout i, half) <- half ^ bit3(i)
  // LDS: three X buffers (the raw tile of chunk c + 1 is transformed under the MFMAs of chunk c, so chunk c + 2 is in flight then) and
  // two U buffers.  A wave issues all its pieces of a chunk at the head of the chunk: the partner wave on the SIMD covers the issue
  // cost, and the pieces get the whole chunk to land before the barrier that drains them.
  auto stage_x = [&](int buf, int cb) {
    char* xs = smem + buf * XBYTES;
    const unsigned xso = (unsigned)cb * (unsigned)HWin * 32u;
#pragma unroll
    for (int r = 0; r < NXR; ++r) {
      const int u = r * NV + wave;
      if ((r + 1) * NV <= NXU || u < NXU)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(x_rs, (__attribute__((address_space(3))) void*)(xs + u * 1024), 16, xvo[r], xso, 0, 0);
    }
  };
  auto stage_u = [&](int buf, int cb) {
    char* us = smem + 3 * XBYTES + buf * (NWU * 1024);
    const unsigned uso = (unsigned)cb * (NWU * 1024u);
#pragma unroll
    for (int r = 0; r < NWR; ++r) {
      const int u = r * NV + wave;  // unit = transform point
      __builtin_amdgcn_raw_ptr_buffer_load_lds(u_rs, (__attribute__((address_space(3))) void*)(us + u * 1024), 16, uvo, uso + u * 1024u, 0, 0);
    }
  };

  // Residual 1 of the workgroup's own output tile: wave w moves tile row w, 8 pieces of 1 KiB = 32 pixels of one channel-block plane
  // (eight whole 128-byte lines), to LDS byte (row * 4 + g) * 2048 + pixel * 32 with the two 16-byte halves of a pixel swapped when
  // bit 3 of the pixel is set (the epilogue's lanes stride 64 B, as the readers of X do).  Rows >= H, pixels >= W and planes that carry
  // no residual get an out-of-range offset.
  auto stage_res = [&]() {
    const __amdgpu_buffer_rsrc_t r_rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.res1 + (long long)n * p.res1_ns), 0, (unsigned)((long long)min(p.cout_blocks, p.res_cb1) * p.H * p.W * 32), 0x00020000);
    const int gy = y0 + wave, pp = lane >> 1;
    const int hsw = (lane & 1) ^ ((pp >> 3) & 1);
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) {
      const int gx = x0 + hp * 32 + pp;
      const unsigned vo = (gy < p.H && gx < p.W) ? (unsigned)((gy * p.W + gx) * 8 + hsw * 4) * 4u : 0xfffffff0u;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = cog * 4 + g;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_rs, (__attribute__((address_space(3))) void*)(smem + ((wave * 4 + g) * 2 + hp) * 1024), 16,
                                                 cb < p.res_cb1 ? vo : 0xfffffff0u, (unsigned)cb * (unsigned)(p.H * p.W) * 32u, 0, 0);
      }
    }
  };

  f32x16 acc[8];  // points 8 HF .. 8 HF + 7
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;

  // byte offset of the first raw pixel this half reads (raw row HF of the patch, column c): tile row 2 prow + HF, tile column
  // 2 j + c, swizzled half
  int xlane[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) xlane[c] = ((2 * prow + HF) * XROW + 2 * j + c) * 32 + ((h ^ (((2 * j + c) >> 3) & 1)) * 16);
  const int ulane = HF * 8 * 1024 + j * 32 + ((h ^ ((j >> 3) & 1)) * 16);

  // V = B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1], as one fixed tree: rows first (tr = B^T d), then columns.
  // This half's two rows of tr: low d0 - d2, d1 + d2; high d2 - d1, d1 - d3
  f32x4 tr[2][4], v[8];
  auto rows = [&](int buf) {
    const char* xb = smem + buf * XBYTES;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 e0 = *(const f32x4*)(xb + xlane[c]);
      const f32x4 e1 = *(const f32x4*)(xb + xlane[c] + XROW * 32);
      const f32x4 e2 = *(const f32x4*)(xb + xlane[c] + 2 * XROW * 32);
      if constexpr (HF == 0) {  // e = d0, d1, d2
        tr[0][c] = e0 - e2;
        tr[1][c] = e1 + e2;
      } else {  // e = d1, d2, d3
        tr[0][c] = e1 - e0;
        tr[1][c] = e0 - e2;
      }
    }
  };
  auto cols = [&](int r) {
    v[r * 4 + 0] = tr[r][0] - tr[r][2];
    v[r * 4 + 1] = tr[r][1] + tr[r][2];
    v[r * 4 + 2] = tr[r][2] - tr[r][1];
    v[r * 4 + 3] = tr[r][1] - tr[r][3];
  };

  const int nchunk = p.cin_blocks;
  // With one chunk rows(0) is not separated from the chunk by a barrier (another wave may still read X buffer 0): no staging then
  const bool res_lds = RES_LDS && p.res_stage && p.res1 != nullptr && nchunk >= 2;
  stage_x(0, 0);
  stage_u(0, 0);
  if (nchunk > 1) stage_x(1, 1);
  __syncthreads();
  WINO_STAMP(1);
  rows(0);
#pragma unroll
  for (int r = 0; r < 2; ++r) cols(r);
  int xb2 = 2 % 3, xb1 = 1;  // X buffers of chunks c + 2 and c + 1
  // one chunk; MORE / MORE2: chunks c + 1 / c + 2 exist (compile-time, so that the body is one straight line the scheduler can
  // interleave: the last two chunks are peeled).  RES: the last chunk of a tile whose residual goes through the LDS.  No wave reads a
  // raw row in it (the rows of chunk nchunk - 1 were read before the barrier of chunk nchunk - 2), it stages neither X nor U, and no
  // LDS read follows the staging point, so the pieces land under its MFMAs and its barrier drains them
  auto chunk = [&](int c, auto more_t, auto more2_t, auto res_t) {
    constexpr bool more = decltype(more_t)::value, more2 = decltype(more2_t)::value, res = decltype(res_t)::value;
    static_assert(!res || (!more && RES_LDS), "the residual is staged in the last chunk only");
    const char* us = smem + 3 * XBYTES + (c & 1) * (NWU * 1024) + ulane;
    f32x4 a[2][4];  // U operands, read one group ahead
#pragma unroll
    for (int q = 0; q < 4; ++q) a[0][q] = *(const f32x4*)(us + q * 1024);
#pragma unroll
    for (int g = 0; g < 2; ++g) {  // four points at a time: dependent MFMAs of one accumulator are four instructions apart
      if (g == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a[1][q] = *(const f32x4*)(us + (4 + q) * 1024);
        if constexpr (more2) stage_x(xb2, c + 2);
        if constexpr (more) stage_u((c + 1) & 1, c + 1);
        if constexpr (res) {
          if (res_lds) stage_res();
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          acc[g * 4 + q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g][q][s], v[g * 4 + q][s], acc[g * 4 + q], 0, 0, 0);
      // the next chunk's operand, behind the MFMAs that read the current one: the raw rows and their row transform under group 0,
      // then V's row 0 once group 0 has been issued
      if constexpr (more) {
        if (g == 0) rows(xb1);
        else cols(0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (more) cols(1);
    __syncthreads();  // drains the LDS-DMA issued in this chunk; frees U buffer c & 1 and the X buffer of chunk c + 1
    xb1 = xb2;
    xb2 = xb2 == 2 ? 0 : xb2 + 1;
  };
  using yes = std::true_type;
  using no = std::false_type;
  for (int c = 0; c + 2 < nchunk; ++c) chunk(c, yes{}, yes{}, no{});
  if (nchunk > 1) chunk(nchunk - 2, yes{}, no{}, no{});
  WINO_STAMP(5);
  chunk(nchunk - 1, no{}, no{}, std::integral_constant<bool, RES_LDS>{});
  WINO_STAMP(2);

  // ---- output transform Y = A^T (M A), A^T = [1 1 1 0; 0 1 -1 -1]: columns first (per transform row: inside the wave), then rows,
  // one fixed tree.  ra[0], ra[1] are transform rows 2 HF, 2 HF + 1
  f32x16 ra[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    ra[r][0] = (acc[r * 4 + 0] + acc[r * 4 + 1]) + acc[r * 4 + 2];
    ra[r][1] = (acc[r * 4 + 1] - acc[r * 4 + 2]) - acc[r * 4 + 3];
  }

  // the row step needs one transform row of the other half: high sends row 2 to low, low sends row 1 to high, through the U buffers
  // (NW = 4: X buffers; dead behind the last chunk's barrier), 8 KiB per wave, each 16-byte store and load contiguous over the lanes
  f32x16 yv[2];  // [dx]
  {
    char* mine = smem + XCH + wave * 8192 + lane * 16;
    const char* theirs = smem + XCH + (HF ? wave - NW : wave + NW) * 8192 + lane * 16;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = ra[1 - HF][c][k * 4 + e];
        *(f32x4*)(mine + (c * 4 + k) * 1024) = o;
      }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      f32x16 rb;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 o = *(const f32x4*)(theirs + (c * 4 + k) * 1024);
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[k * 4 + e] = o[e];
      }
      if constexpr (HF == 0) yv[c] = (ra[0][c] + ra[1][c]) + rb;  // (ra0 + ra1) + ra2
      else yv[c] = (rb - ra[0][c]) - ra[1][c];                    // (ra1 - ra2) - ra3
    }
  }

  WINO_STAMP(3);

  // ---- epilogue (that of conv_tile_f32): bias, LeakyReLU, alpha, residual scale-adds, 16-byte CB8 stores.  This half's output row
  // is dy = HF.  STAGED: residual 1 comes from the tile stage_res() brought in (same value, same expression), and the loads of
  // residual 2 (one conv5 in three has it; there is no room for a second tile) are all issued in front of the first store: they may
  // alias the destination, so the compiler keeps each behind the store before it otherwise.  A lane loads only what it stores itself.
  // The accumulators are dead here: the 32 registers are free
  const long long HW = (long long)p.H * p.W;
  const int y = y0 + 2 * prow + HF;
  const int rlane = (2 * prow + HF) * 8192 + j * 64 + ((h ^ ((j >> 2) & 1)) * 16);
  auto epilogue = [&](auto staged_t) {
    constexpr bool staged = decltype(staged_t)::value;
    f32x4 bv[4];  // read once in front of the stores: a load behind a store waits for the store with it (one counter)
    if (p.bias) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (cog * 4 + g < p.cout_blocks) bv[g] = *(const f32x4*)(p.bias + (cog * 4 + g) * 8 + h * 4);
    }
    f32x4 r2[2][4];
    if constexpr (staged) {
      if (p.res2) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int x = x0 + 2 * j + dx;
          if (y >= p.H || x >= p.W) continue;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int cb = cog * 4 + g;
            if (cb >= p.cout_blocks || cb >= p.res_cb1) continue;
            r2[dx][g] = *(const f32x4*)(p.res2 + (long long)n * p.res2_ns + (cb * HW + (long long)y * p.W + x) * 8 + h * 4);
          }
        }
      }
    }
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int x = x0 + 2 * j + dx;
      if (y >= p.H || x >= p.W) continue;
      const long long pixoff = (long long)y * p.W + x;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = cog * 4 + g;
        if (cb >= p.cout_blocks) continue;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = yv[dx][g * 4 + e];
        const long long off = (cb * HW + pixoff) * 8 + h * 4;
        if (p.bias) o += bv[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = o[e] > 0.f ? o[e] : o[e] * p.slope;
        o *= p.alpha;
        if constexpr (staged) {
          if (cb < p.res_cb1) o += p.beta1 * *(const f32x4*)(smem + rlane + g * 2048 + dx * 32);
          if (p.res2 && cb < p.res_cb1) o += p.beta2 * r2[dx][g];
        } else {
          if (p.res1 && cb < p.res_cb1) o += p.beta1 * *(const f32x4*)(p.res1 + (long long)n * p.res1_ns + off);
          if (p.res2 && cb < p.res_cb1) o += p.beta2 * *(const f32x4*)(p.res2 + (long long)n * p.res2_ns + off);
        }
        *(f32x4*)(p.out + (long long)n * p.out_ns + off) = o;
      }
    }
  };
  if constexpr (RES_LDS) {
    if (res_lds) epilogue(yes{});
    else epilogue(no{});
  } else {
    epilogue(no{});
  }
  WINO_STAMP(4);
}

template <int NW>
__global__ __launch_bounds__(NW * 128, 2) void conv_wino_f32_kernel(const WinoParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave < NW) conv_wino_tile_f32<NW, 0>(p, smem, wave);
  else conv_wino_tile_f32<NW, 1>(p, smem, wave);
}

#ifdef SR_WINO_STAMP
unsigned long long* g_wino_stamps = nullptr;
#endif

template <int NW>
int launch_wino(const WinoParams& p0, const sr_conv3x3_desc* d, hipStream_t stream) {
  WinoParams p = p0;
#ifdef SR_WINO_STAMP
  p.stamps = g_wino_stamps;
#endif
  p.tiles_x = sr::cdiv(p.W, 64);
  p.tiles_y = sr::cdiv(p.H, 2 * NW);
  constexpr int lds = wino_lds_bytes<NW>();
  auto kern = conv_wino_f32_kernel<NW>;
  if (int rc = sr::ensure_dynamic_lds((const void*)kern, lds)) return rc;
  const int groups = d->cout / 32;
  const bool prof = sr::prof_on();
  if (prof) {
    sr_launch_record r = {};
    r.kernel_id = NW == 4 ? 106 : NW == 2 ? 107 : 108;
    r.cin = d->cin_real > 0 ? d->cin_real : d->cin_pad;
    r.cout = d->cout;
    r.n = d->n;
    r.h = p.H;
    r.w = p.W;
    const double px = (double)d->n * p.H * p.W;
    const double patches = (double)d->n * ((p.H + 1) / 2) * ((p.W + 1) / 2);
    r.flops = 2.0 * 16 * d->cin_pad * d->cout * patches;  // executed MFMA work: 16 points per (cin, cout, patch)
    double fl = (double)d->n * p.in_h * p.in_w * r.cin + px * r.cout;  // source once, destination once
    if (d->res1) fl += px * r.cout;
    if (d->res2) fl += px * r.cout;
    r.bytes = 4.0 * fl;
    sr::prof_begin(stream, r);
  }
  hipLaunchKernelGGL(kern, dim3(p.tiles_x * p.tiles_y * d->n, groups), dim3(NW * 128), lds, stream, p);
  if (prof) sr::prof_end(stream);
  SR_CHECK_LAUNCH("conv_wino_f32 launch");
  return SR_OK;
}

// 0 = off, 1 = on (default), 2 / 3 / 4 = on with the tile variant forced (NW = 4 / 2 / 1) at every size.
// SR_F32_WINOGRAD in the environment, read once at first use, sets the initial value.
int g_wino_mode = -1;

// Residual 1 through the LDS (NW = 2, 1; two chunks or more): 1 = on (default), 0 = off: the epilogue loads it from memory.  Same
// bits either way.  SR_F32_WINO_RES_STAGE in the environment, read once at first use, sets the initial value.
int g_wino_res_stage = -1;

int wino_res_stage() {
  if (g_wino_res_stage < 0) {
    const char* e = getenv("SR_F32_WINO_RES_STAGE");
    g_wino_res_stage = (e && *e) ? (atoi(e) != 0) : 1;
  }
  return g_wino_res_stage;
}

}  // namespace

namespace sr {

int wino_f32_mode() {
  if (g_wino_mode < 0) {
    const char* e = getenv("SR_F32_WINOGRAD");
    g_wino_mode = (e && *e) ? atoi(e) : 1;
    if (g_wino_mode < 0 || g_wino_mode > 4) g_wino_mode = 1;
  }
  return g_wino_mode;
}

bool wino_f32_weights_eligible(int cout, int cin) { return cin >= 8 && cout > 0 && cout % 32 == 0; }

size_t wino_f32_image_floats(int cout, int cin_pad) { return (size_t)cout * cin_pad * 16; }

// SR_OK: launched.  SR_WINO_NOT_ELIGIBLE: nothing launched, the caller runs the direct kernels.  < 0: error.
int conv3x3_wino_f32(const sr_conv3x3_desc* d, const float* image, hipStream_t stream, bool any_size) {
  SR_CHECK_ARG(d != nullptr && image != nullptr, "conv3x3_wino_f32: null argument");
  SR_CHECK_ARG(d->in && d->out, "conv3x3_wino_f32: null in/out");
  SR_CHECK_ARG(d->cin_pad > 0 && d->cin_pad % 8 == 0, "conv3x3_wino_f32: cin_pad=%d must be a positive multiple of 8", d->cin_pad);
  SR_CHECK_ARG(d->cout > 0 && d->n > 0 && d->in_h > 0 && d->in_w > 0, "conv3x3_wino_f32: bad shape");
  SR_CHECK_ARG(((uintptr_t)d->in | (uintptr_t)image | (uintptr_t)d->out | (uintptr_t)d->res1 | (uintptr_t)d->res2 | (uintptr_t)d->bpacked) % 16 == 0,
               "conv3x3_wino_f32: pointers must be 16-byte aligned");
  const int cin = d->cin_real > 0 ? d->cin_real : d->cin_pad;
  if (!wino_f32_weights_eligible(d->cout, cin) || d->out_nchw || d->accumulate || d->mask_src || d->s2_channels || d->out_unshuffle2 ||
      d->res1_u2 || d->res1_keep_sign || (d->upsample != 0 && d->upsample != 1))
    return SR_WINO_NOT_ELIGIBLE;
  WinoParams p = {};
  p.in = d->in;
  p.u = image;
  p.bias = d->bpacked;
  p.out = d->out;
  p.res1 = d->res1;
  p.res2 = d->res2;
  p.in_ns = d->in_img_stride;
  p.out_ns = d->out_img_stride;
  p.res1_ns = d->res1_img_stride;
  p.res2_ns = d->res2_img_stride;
  p.cin_blocks = d->cin_pad / 8;
  p.cout_blocks = d->cout / 8;
  p.in_h = d->in_h;
  p.in_w = d->in_w;
  p.src_shift = d->upsample ? 1 : 0;
  p.H = d->in_h << p.src_shift;
  p.W = d->in_w << p.src_shift;
  p.res_cb1 = d->res_cbn > 0 ? d->res_cbn : (1 << 30);
  p.res_stage = wino_res_stage();
  p.slope = d->act_slope;
  p.alpha = d->alpha;
  p.beta1 = d->beta1;
  p.beta2 = d->beta2;
  // 32-bit plane offsets and buffer ranges (bytes)
  const long long blocks = p.cout_blocks > p.cin_blocks ? p.cout_blocks : p.cin_blocks;
  if ((long long)p.H * p.W * 32 * blocks >= (1ll << 31) || (long long)p.in_h * p.in_w * 32 * blocks >= (1ll << 31))
    return SR_WINO_NOT_ELIGIBLE;
  const int mode = wino_f32_mode();
  // Below 128 x 128 output pixels per image a launch of single images cannot give every SIMD a 32-patch x 32-cout wave: the direct
  // kernels, which split a 32-cout tile over four waves, are faster there.  By H x W alone: never by n, so that a batched call and
  // a single-image call take the same arithmetic.
  if (!any_size && mode < 2 && (long long)p.H * p.W < 128 * 128) return SR_WINO_NOT_ELIGIBLE;
  const long long rows2 = cdiv(p.H, 4), rows1 = cdiv(p.H, 2);
  const long long per_row = (long long)cdiv(p.W, 64) * d->n * (d->cout / 32) * launch_concurrency();
  if (per_row * rows1 >= (1ll << 31)) return SR_WINO_NOT_ELIGIBLE;
  // every variant gives the same bits.  A launch that fills the chip takes NW = 2: two independent four-wave workgroups per CU (two
  // waves per SIMD, as one eight-wave NW = 4 workgroup gives) whose barriers and tile boundaries drift apart measured 3.3 % faster
  // than NW = 4 at the benchmark's size, so NW = 4 runs only when forced.  Below that, the tallest tile that still gives every CU a
  // workgroup
  const int nw = mode >= 2 ? (mode == 2 ? 4 : mode == 3 ? 2 : 1) : rows2 * per_row >= 256 ? 2 : 1;
  return nw == 4 ? launch_wino<4>(p, d, stream) : nw == 2 ? launch_wino<2>(p, d, stream) : launch_wino<1>(p, d, stream);
}

}  // namespace sr

extern "C" int sr_dev_set_wino_f32(int mode) {  // development switch (not in the ABI header)
  g_wino_mode = (mode >= 0 && mode <= 4) ? mode : 1;
  return SR_OK;
}

extern "C" int sr_dev_set_wino_res_stage(int on) {  // development switch (not in the ABI header)
  g_wino_res_stage = on != 0;
  return SR_OK;
}

#ifdef SR_WINO_STAMP
// diagnostic build only: device buffer of 8 values per workgroup of the next launches, or null
extern "C" int sr_dev_set_wino_stamps(unsigned long long* buf) {
  g_wino_stamps = buf;
  return SR_OK;
}
#endif

// Test hooks: one conv on the Winograd kernel (returns 1 = not eligible, nothing launched), and the weight image of one conv.
extern "C" int sr_dev_conv3x3_wino_f32(const sr_conv3x3_desc* d, const float* wino_image, void* stream) {
  return sr::conv3x3_wino_f32(d, wino_image, (hipStream_t)stream, true);
}

extern "C" size_t sr_dev_conv3x3_wino_packed_floats(int cout, int cin_pad) {
  return (cout > 0 && cin_pad > 0 && cout % 32 == 0 && cin_pad % 8 == 0) ? sr::wino_f32_image_floats(cout, cin_pad) : 0;
}

// weight: OIHW [cout][cin][3][3] on the device; (first_seg, seg) as sr_conv3x3_pack_f32; wino_image: packed_floats floats,
// followed by sr::pack_table_bytes(1) bytes for the pack table
extern "C" int sr_dev_conv3x3_wino_pack_f32(const float* weight, int cout, int cin, int first_seg, int seg, float* wino_image,
                                            void* stream) {
  SR_CHECK_ARG(weight && wino_image && sr::wino_f32_weights_eligible(cout, cin), "sr_dev_conv3x3_wino_pack_f32: bad argument");
  const int cin_pad = sr_conv3x3_cin_pad(cin, first_seg, seg);
  SR_CHECK_ARG(cin_pad > 0, "sr_dev_conv3x3_wino_pack_f32: cin=%d is not first_seg=%d + k*seg=%d", cin, first_seg, seg);
  std::vector<sr::PackEntry> tab(1);
  sr::PackEntry& e = tab[0];
  e = sr::PackEntry{};
  e.kind = 3;
  e.w[0] = weight;
  e.out = wino_image;
  e.cout = cout;
  e.cin = cin;
  e.first_seg = first_seg;
  e.seg = seg > 0 ? seg : 1;
  e.cin_pad = cin_pad;
  return sr::pack_table_run(tab, wino_image, sr::wino_f32_image_floats(cout, e.cin_pad) * sizeof(float), false, (hipStream_t)stream);
}

extern "C" size_t sr_dev_conv3x3_wino_pack_bytes(int cout, int cin_pad) {  // image + table: what sr_dev_conv3x3_wino_pack_f32 writes
  const size_t f = sr_dev_conv3x3_wino_packed_floats(cout, cin_pad);
  return f ? f * sizeof(float) + sr::pack_table_bytes(1) : 0;
}
