// What the CB16 MFMA kernels of the EDVR bf16 forward share (dcn_ops_bf16.hip, edvr_ops_bf16.hip): the vector types, the bf16
// conversions and the tile epilogue.  The epilogue restates the bf16 epilogue of conv_bf16.hip (epilogue_cb16) for a conv with
// bias and LeakyReLU only: the same operations in the same order per element, the same round-to-nearest-even conversion, the
// same v_permlane32_swap so that every lane stores 16 B = 8 consecutive channels.
#pragma once
#include "sr_internal.h"

namespace cb16 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
// element e (0..7) of 8 bf16 held as four dwords
__device__ __forceinline__ float bf_at(const u32x4& v, int e) { return (e & 1) ? bf_hi(v[e >> 1]) : bf_lo(v[e >> 1]); }
__device__ __forceinline__ unsigned f2bf2(float lo, float hi) {  // two round-to-nearest-even conversions, packed
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  bf16x2 t = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, t);
}
__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
  return u32x4{f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]), f2bf2(v[6], v[7])};
}
__device__ __forceinline__ float sigmoidf_(float s) { return 1.f / (1.f + expf(-s)); }

// Accumulators of v_mfma_f32_32x32x16_bf16 tiles: acc[c][r] = 32 couts x 32 pixels, pixel on the lane (j = lane & 31), couts
// 8 g + 4 h + e in register 4 g + e (h = lane >> 5).  Writes bf16(lrelu(acc + bias)) for the pixel `pix[r]` (an index into one
// block plane of `plane` pixels; < 0: nothing is written) of every block below cout_blocks.  `bias`: fp32 [cout padded to 32] or
// null.  Couts beyond the real ones meet zero weights and zero bias, so pad channels come out as zero.
template <int COT, int PT>
__device__ __forceinline__ void epilogue(f32x16 (&acc)[COT][PT], const float* bias, float slope, char* out_n, long long plane,
                                         const long long (&pix)[PT], int cog, int cout_blocks, int h) {
  auto swap_halves = [](u32x4& t) {  // t[0..1].upper-lanes <-> t[2..3].lower-lanes
    auto r0 = __builtin_amdgcn_permlane32_swap(t[0], t[2], false, false);
    auto r1 = __builtin_amdgcn_permlane32_swap(t[1], t[3], false, false);
    t = u32x4{r0[0], r1[0], r0[1], r1[1]};
  };
  f32x4 bv[COT][4];
#pragma unroll
  for (int c = 0; c < COT; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      bv[c][g] = bias ? *(const f32x4*)(bias + (cog * COT + c) * 32 + g * 8 + h * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < PT; ++r) {
#pragma unroll
    for (int c = 0; c < COT; ++c) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {  // the two 16-channel blocks of this 32-cout tile
        const int cb = (cog * COT + c) * 2 + m;
        float v[8];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float t = acc[c][r][(2 * m + q) * 4 + e];
            if (bias) t += bv[c][2 * m + q][e];
            v[q * 4 + e] = t > 0.f ? t : t * slope;
          }
        u32x4 o = pack8(v);
        swap_halves(o);  // the swap involves every lane of the wave: it stays outside the bounds test
        if (cb < cout_blocks && pix[r] >= 0)
          *(__attribute__((address_space(1))) u32x4*)(out_n + ((cb * plane + pix[r]) * 16 + h * 8) * 2) = o;
      }
    }
  }
}

inline bool aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if ((uintptr_t)q % 16) return false;
  return true;
}

}  // namespace cb16
