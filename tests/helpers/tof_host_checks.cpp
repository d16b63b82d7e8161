// Stand-alone driver for the host-side code of tof_ops.hip: the argument checks and the size query of its entry points, built
// with the host sanitizers and run on a machine without a GPU.  Every call below returns before anything is launched.  The few
// library services that translation unit uses are stubbed here.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       image_restoration_amd/csrc/tof_ops.hip tests/helpers/tof_host_checks.cpp \
//       -o tof_host_checks && ./tof_host_checks
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../image_restoration_amd/csrc/sr_internal.h"
#include "../../include/sr_hip_tof.h"

static char g_err[512];
namespace sr {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
bool prof_on() { return false; }
void prof_begin(hipStream_t, const sr_launch_record&) {}
void prof_end(hipStream_t) {}
int ensure_dynamic_lds(const void*, int) { return SR_ELAUNCH; }  // never reached: every call below is refused before it
}  // namespace sr

static int failures = 0;
static int checks = 0;
// the call must be refused with SR_EINVAL and a message that names the entry point and contains `needle`
#define REFUSED(call, name, needle)                                                                     \
  do {                                                                                                  \
    g_err[0] = 0;                                                                                       \
    ++checks;                                                                                           \
    const int rc__ = (call);                                                                            \
    if (rc__ != SR_EINVAL || !strstr(g_err, name) || !strstr(g_err, needle)) {                          \
      printf("FAILED line %d: %s -> %d (last error: %s)\n", __LINE__, #call, rc__, g_err);              \
      ++failures;                                                                                       \
    }                                                                                                   \
  } while (0)
#define EXPECT(cond)                                    \
  do {                                                  \
    ++checks;                                           \
    if (!(cond)) {                                      \
      printf("FAILED line %d: %s\n", __LINE__, #cond);  \
      ++failures;                                       \
    }                                                   \
  } while (0)

int main() {
  float* const P = (float*)256;   // fake aligned addresses: nothing is launched, so nothing is dereferenced
  float* const Q = (float*)4096;
  float* const U = (float*)4100;  // 4-byte aligned only
  const float m3[3] = {0.5f, 0.5f, 0.5f};

  // ---- size query: exactly two pairs are served
  for (int cin = -2; cin < 80; ++cin)
    for (int cout = -2; cout < 80; ++cout) {
      const size_t f = sr_tof_conv9x9_packed_floats(cout, cin);
      const bool served = cout == 64 && (cin == 21 || cin == 64);
      EXPECT(f == (served ? (size_t)((cin + 7) / 8) * 81 * 512 + 64 : 0));
      if (!served) {
        REFUSED(sr_tof_conv9x9_pack_f32(P, nullptr, cout, cin, Q, nullptr), "sr_tof_conv9x9_pack_f32", "supported: (21, 64), (64, 64)");
        sr_tof_conv9x9_desc d = {P, 64ll * 64, cin, cout, 1, 8, 8, Q, Q, 64ll * 64, 0};
        REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "supported: (21, 64), (64, 64)");
      }
    }
  REFUSED(sr_tof_conv9x9_pack_f32(nullptr, nullptr, 64, 64, Q, nullptr), "sr_tof_conv9x9_pack_f32", "null");
  REFUSED(sr_tof_conv9x9_pack_f32(P, nullptr, 64, 21, nullptr, nullptr), "sr_tof_conv9x9_pack_f32", "null");
  REFUSED(sr_tof_conv9x9_pack_f32(P, nullptr, 64, 21, U, nullptr), "sr_tof_conv9x9_pack_f32", "16-byte aligned");

  // ---- conv descriptor
  const sr_tof_conv9x9_desc ok = {P, 24ll * 64, 21, 64, 1, 8, 8, Q, Q, 64ll * 64, 0};
  REFUSED(sr_tof_conv9x9_f32(nullptr, nullptr), "sr_tof_conv9x9_f32", "null descriptor");
  sr_tof_conv9x9_desc d = ok;
  d.in = nullptr;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "null in / packed / out");
  d = ok, d.packed = nullptr;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "null in / packed / out");
  d = ok, d.out = nullptr;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "null in / packed / out");
  for (int bad = -1; bad <= 0; ++bad) {
    d = ok, d.n = bad;
    REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "bad shape");
    d = ok, d.h = bad;
    REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "bad shape");
    d = ok, d.w = bad;
    REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "bad shape");
  }
  d = ok, d.in = U;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "16-byte aligned");
  d = ok, d.out = U;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "16-byte aligned");
  d = ok, d.packed = U;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "16-byte aligned");
  d = ok, d.in_img_stride += 2;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "multiples of 4 floats");
  d = ok, d.out_img_stride += 1;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "multiples of 4 floats");
  for (int relu = -1; relu <= 2; relu += 3) {
    d = ok, d.relu = relu;
    REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "relu must be 0 or 1");
  }
  d = ok, d.h = 1 << 12, d.w = 1 << 12, d.in_img_stride = d.out_img_stride = 1ll << 40;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "too large");
  d = ok, d.h = 0x7fffffff, d.w = 0x7fffffff, d.in_img_stride = d.out_img_stride = 1ll << 62;   // no overflow on the way
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "too large");
  d = ok, d.in_img_stride = 16 * 64;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "smaller than the image");
  d = ok, d.out_img_stride = 56 * 64;
  REFUSED(sr_tof_conv9x9_f32(&d, nullptr), "sr_tof_conv9x9_f32", "smaller than the image");

  // ---- level input
  const char* L = "sr_tof_level_input_f32";
  const long long s3 = 3 * 64;
  REFUSED(sr_tof_level_input_f32(nullptr, s3, P, s3, 1, 1, Q, Q, Q, 2, 8, 8, nullptr), L, "null");
  REFUSED(sr_tof_level_input_f32(P, s3, nullptr, s3, 1, 1, Q, Q, Q, 2, 8, 8, nullptr), L, "null");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, nullptr, Q, 2, 8, 8, nullptr), L, "null");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, Q, nullptr, 2, 8, 8, nullptr), L, "null");
  for (int bad : {0, -1, 65536}) REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, Q, Q, bad, 8, 8, nullptr), L, "bad shape");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, Q, Q, 2, 0, 8, nullptr), L, "bad shape");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, Q, Q, 2, 8, -3, nullptr), L, "bad shape");
  for (int group : {0, -6, 4}) REFUSED(sr_tof_level_input_f32(P, 7 * s3, P, 7 * s3, group, 0, Q, Q, Q, 6, 8, 8, nullptr), L, "multiple of group");
  for (int skip : {-1, 7}) REFUSED(sr_tof_level_input_f32(P, 7 * s3, P, 7 * s3, 6, skip, Q, Q, Q, 6, 8, 8, nullptr), L, "multiple of group");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, Q, Q, 2, 7, 8, nullptr), L, "must be even");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, Q, Q, 2, 8, 9, nullptr), L, "must be even");
  REFUSED(sr_tof_level_input_f32(P, 1ll << 40, P, 1ll << 40, 1, 1, nullptr, Q, Q, 2, 1 << 14, 1 << 14, nullptr), L, "too large");
  REFUSED(sr_tof_level_input_f32(P, 1ll << 62, P, 1ll << 62, 1, 1, nullptr, Q, Q, 2, 0x7fffffff, 0x7fffffff, nullptr), L, "too large");
  REFUSED(sr_tof_level_input_f32(P, s3 - 1, P, s3, 1, 1, Q, Q, Q, 2, 8, 8, nullptr), L, "group stride");
  REFUSED(sr_tof_level_input_f32(P, 7 * s3, P, 6 * s3, 6, 3, Q, Q, Q, 6, 8, 8, nullptr), L, "group stride");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, U, Q, Q, 2, 8, 8, nullptr), L, "16-byte aligned");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, U, Q, 2, 8, 8, nullptr), L, "16-byte aligned");
  REFUSED(sr_tof_level_input_f32(P, s3, P, s3, 1, 1, Q, Q, U, 2, 8, 8, nullptr), L, "16-byte aligned");

  // ---- aligned stack
  const char* A = "sr_tof_align_f32";
  REFUSED(sr_tof_align_f32(nullptr, Q, 8 * 64, Q, 24 * 64, 1, 3, 8, 8, nullptr), A, "null");
  REFUSED(sr_tof_align_f32(P, nullptr, 8 * 64, Q, 24 * 64, 1, 3, 8, 8, nullptr), A, "null");
  REFUSED(sr_tof_align_f32(P, Q, 8 * 64, nullptr, 24 * 64, 1, 3, 8, 8, nullptr), A, "null");
  for (int bad : {0, -1, 65536}) REFUSED(sr_tof_align_f32(P, Q, 8 * 64, Q, 24 * 64, bad, 3, 8, 8, nullptr), A, "bad shape");
  REFUSED(sr_tof_align_f32(P, Q, 8 * 64, Q, 24 * 64, 1, 3, 0, 8, nullptr), A, "bad shape");
  REFUSED(sr_tof_align_f32(P, Q, 8 * 64, Q, 24 * 64, 1, 3, 8, -1, nullptr), A, "bad shape");
  for (int r : {-1, 7, 100}) REFUSED(sr_tof_align_f32(P, Q, 8 * 64, Q, 24 * 64, 1, r, 8, 8, nullptr), A, "not one of the 7 frames");
  REFUSED(sr_tof_align_f32(P, Q, 1ll << 40, Q, 1ll << 40, 1, 3, 1 << 13, 1 << 13, nullptr), A, "too large");
  REFUSED(sr_tof_align_f32(P, Q, 1ll << 62, Q, 1ll << 62, 1, 3, 0x7fffffff, 0x7fffffff, nullptr), A, "too large");
  REFUSED(sr_tof_align_f32(P, U, 8 * 64, Q, 24 * 64, 1, 3, 8, 8, nullptr), A, "16-byte aligned");
  REFUSED(sr_tof_align_f32(P, Q, 8 * 64, U, 24 * 64, 1, 3, 8, 8, nullptr), A, "16-byte aligned");
  REFUSED(sr_tof_align_f32(P, Q, 8 * 64 + 2, Q, 24 * 64, 1, 3, 8, 8, nullptr), A, "multiples of 4 floats");
  REFUSED(sr_tof_align_f32(P, Q, 8 * 64, Q, 24 * 64 + 1, 1, 3, 8, 8, nullptr), A, "multiples of 4 floats");
  REFUSED(sr_tof_align_f32(P, Q, 8 * 64 - 4, Q, 24 * 64, 1, 3, 8, 8, nullptr), A, "smaller than the image");
  REFUSED(sr_tof_align_f32(P, Q, 8 * 64, Q, 24 * 64 - 4, 1, 3, 8, 8, nullptr), A, "smaller than the image");

  // ---- finish
  const char* F = "sr_tof_finish_f32";
  REFUSED(sr_tof_finish_f32(nullptr, 8 * 64, P, s3, P, 1, 8, 8, m3, m3, nullptr), F, "null");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64, nullptr, s3, P, 1, 8, 8, m3, m3, nullptr), F, "null");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64, P, s3, nullptr, 1, 8, 8, m3, m3, nullptr), F, "null");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64, P, s3, P, 1, 8, 8, nullptr, m3, nullptr), F, "null");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64, P, s3, P, 1, 8, 8, m3, nullptr, nullptr), F, "null");
  for (int bad : {0, -1, 65536}) REFUSED(sr_tof_finish_f32(Q, 8 * 64, P, s3, P, bad, 8, 8, m3, m3, nullptr), F, "bad shape");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64, P, s3, P, 1, 0, 8, m3, m3, nullptr), F, "bad shape");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64, P, s3, P, 1, 8, 0, m3, m3, nullptr), F, "bad shape");
  REFUSED(sr_tof_finish_f32(Q, 1ll << 40, P, 1ll << 40, P, 1, 1 << 14, 1 << 14, m3, m3, nullptr), F, "too large");
  REFUSED(sr_tof_finish_f32(Q, 1ll << 62, P, 1ll << 62, P, 1, 0x7fffffff, 0x7fffffff, m3, m3, nullptr), F, "too large");
  REFUSED(sr_tof_finish_f32(U, 8 * 64, P, s3, P, 1, 8, 8, m3, m3, nullptr), F, "16-byte aligned");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64 + 2, P, s3, P, 1, 8, 8, m3, m3, nullptr), F, "multiple of 4 floats");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64 - 4, P, s3, P, 1, 8, 8, m3, m3, nullptr), F, "smaller than the image");
  REFUSED(sr_tof_finish_f32(Q, 8 * 64, P, s3 - 1, P, 1, 8, 8, m3, m3, nullptr), F, "smaller than the image");

  printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
