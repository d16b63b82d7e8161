// The order-free sum of the deterministic gradients (vsr_det_ops.hip, dcn_det_ops.hip): terms are scaled by 2^k, rounded
// to integers and added with 64-bit integer atomics, so the sum does not depend on the order in which the adds arrive, and is
// scaled back with one rounding.  k comes from the exponent of a per-image maximum M, itself taken order-free as the unsigned
// maximum of sign-cleared bit patterns (a NaN's bits lie above kInfBits, so it wins), and from the level L = ceil(log2(terms per
// element)): with k = 61 - e - L a term is at most 2^(61 - L) and a sum at most 2^61.
//
// Here is what the two files share word for word.  Which tensors feed M, how k is formed from one or two exponents and what an
// all-zero or non-finite M means for the result are theirs.
#pragma once
#include <math.h>

#include "sr_internal.h"

namespace fixsum {

// ------------------------------------------------------------------------------------------------------------------ device
constexpr unsigned kInfBits = 0x7f800000u;

// ilogb(M) + 1 from the bits of M (finite, not zero; a denormal has its exponent from its leading bit)
__device__ __forceinline__ int exp_of(unsigned mbits) {
  const int ex = (int)(mbits >> 23);
  return (ex ? ex - 127 : (31 - __clz((int)mbits)) - 149) + 1;
}

// m joined with the maximum of the sign-cleared bit patterns of four floats
__device__ __forceinline__ unsigned max_abs_bits(unsigned m, const uint4 v) {
  return max(max(m, v.x & 0x7fffffffu), max(v.y & 0x7fffffffu, max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
}

// A lane's maximum over a contiguous run of 16-byte quads that the x dimension of the grid walks, 256 threads a workgroup
__device__ __forceinline__ unsigned walk_max(const uint4* src, long long quads) {
  unsigned m = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) m = max_abs_bits(m, src[i]);
  return m;
}

__device__ __forceinline__ unsigned wave_max(unsigned m) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, s));
  return m;
}

// One integer atomic per wave, and none for a zero maximum (the word was cleared)
__device__ __forceinline__ void publish_max(unsigned* word, unsigned wave_m) {
  if ((threadIdx.x & 63) == 0 && wave_m) atomicMax(word, wave_m);
}

__device__ __forceinline__ void add_term(unsigned long long* acc, double term, int k) {
  atomicAdd(acc, (unsigned long long)llrint(ldexp(term, k)));
}

__device__ __forceinline__ double scaled_back(long long acc, int k) { return ldexp((double)acc, -k); }

// -------------------------------------------------------------------------------------------------------------------- host
// ceil(log2(count))
inline int level_of(long long count) {
  int L = 0;
  while ((1ll << L) < count) ++L;
  return L;
}

// The workspace: the accumulators, then the scale words, each region rounded up to 256 bytes
struct Carve {
  size_t acc_bytes, scale_bytes;
  size_t total() const { return acc_bytes + scale_bytes; }
};

inline Carve carve(size_t acc_bytes, size_t scale_bytes) { return {sr::align_up(acc_bytes, 256), sr::align_up(scale_bytes, 256)}; }

// Refuses a workspace that is misaligned, missing or smaller than the carve (query_name: the entry point's size query), then
// clears it in stream order
inline int check_and_clear(const char* who, const char* query_name, void* workspace, size_t workspace_bytes, const Carve& c,
                           hipStream_t stream) {
  SR_CHECK_ARG(((uintptr_t)workspace & 255u) == 0, "%s: the workspace must be 256-byte aligned", who);
  if (!workspace || workspace_bytes < c.total()) {
    sr::set_error("%s: workspace of %zu bytes, %zu needed (%s)", who, workspace ? workspace_bytes : (size_t)0, c.total(), query_name);
    return SR_ENOSPACE;
  }
  if (hipMemsetAsync(workspace, 0, c.total(), stream) != hipSuccess) {
    sr::set_error("%s: clearing the workspace: %s", who, hipGetErrorString(hipGetLastError()));
    return SR_ELAUNCH;
  }
  return SR_OK;
}

}  // namespace fixsum
