// Stand-alone driver for the host-side code of degrade_ops.hip: the argument checks of its six entry points, built with the host
// sanitizers and run on a machine without a GPU.  Every call below returns before anything is launched.  The few library
// services that translation unit uses are stubbed here.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       image_restoration_amd/csrc/degrade_ops.hip tests/helpers/degrade_host_checks.cpp \
//       -o degrade_host_checks && ./degrade_host_checks
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../image_restoration_amd/csrc/sr_internal.h"
#include "../../include/sr_hip_degrade.h"

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

static float* const P = (float*)256;
static float* const Q = (float*)4096;
static int32_t* const S = (int32_t*)512;

int main() {
  const char* f = "sr_filter2d_f32";
  REFUSED(sr_filter2d_f32(nullptr, P, Q, 1, 3, 16, 16, 3, 1, nullptr), f, "null");
  REFUSED(sr_filter2d_f32(P, nullptr, Q, 1, 3, 16, 16, 3, 1, nullptr), f, "null");
  REFUSED(sr_filter2d_f32(P, P, nullptr, 1, 3, 16, 16, 3, 1, nullptr), f, "null");
  REFUSED(sr_filter2d_f32(P, P, Q, 0, 3, 16, 16, 3, 1, nullptr), f, "bad shape");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 0, 16, 16, 3, 1, nullptr), f, "bad shape");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 0, 16, 3, 1, nullptr), f, "bad shape");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 16, -1, 3, 1, nullptr), f, "bad shape");
  REFUSED(sr_filter2d_f32(P, P, Q, 1 << 15, 3, 16, 16, 3, 1, nullptr), f, "bad shape");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 1 << 16, 1 << 16, 3, 1, nullptr), f, "bad shape");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 16, 16, 4, 1, nullptr), f, "not supported");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 16, 16, 0, 1, nullptr), f, "not supported");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 16, 16, -3, 1, nullptr), f, "not supported");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 64, 64, 23, 1, nullptr), f, "not supported");
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 10, 64, 21, 1, nullptr), f, "too small");   // H = k / 2
  REFUSED(sr_filter2d_f32(P, P, Q, 1, 3, 64, 3, 7, 1, nullptr), f, "too small");     // W = k / 2
  REFUSED(sr_filter2d_f32(P, P, Q, 3, 3, 16, 16, 3, 2, nullptr), f, "kernel_batch");
  REFUSED(sr_filter2d_f32(P, P, Q, 3, 3, 16, 16, 3, 0, nullptr), f, "kernel_batch");
  REFUSED(sr_filter2d_f32(P, P, P, 1, 3, 16, 16, 3, 1, nullptr), f, "must not be x");

  const char* r = "sr_resize_bilinear_f32";
  REFUSED(sr_resize_bilinear_f32(nullptr, nullptr, Q, nullptr, 1, 3, 8, 8, 4, 4, nullptr), r, "null");
  REFUSED(sr_resize_bilinear_f32(P, S, nullptr, S, 1, 3, 8, 8, 4, 4, nullptr), r, "null");
  REFUSED(sr_resize_bilinear_f32(P, nullptr, Q, nullptr, 0, 3, 8, 8, 4, 4, nullptr), r, "bad shape");
  REFUSED(sr_resize_bilinear_f32(P, nullptr, Q, nullptr, 1, 3, 0, 8, 4, 4, nullptr), r, "bad shape");
  REFUSED(sr_resize_bilinear_f32(P, nullptr, Q, nullptr, 1, 3, 8, 8, 4, 0, nullptr), r, "bad shape");
  REFUSED(sr_resize_bilinear_f32(P, nullptr, Q, nullptr, 1, 3, 8, 8, -4, 4, nullptr), r, "bad shape");
  REFUSED(sr_resize_bilinear_f32(P, nullptr, Q, nullptr, 1 << 16, 1, 8, 8, 4, 4, nullptr), r, "bad shape");
  REFUSED(sr_resize_bilinear_f32(P, nullptr, P, nullptr, 1, 3, 8, 8, 4, 4, nullptr), r, "must not be src");

  const char* n = "sr_add_gaussian_noise_f32";
  REFUSED(sr_add_gaussian_noise_f32(nullptr, P, nullptr, P, nullptr, Q, 1, 3, 8, 8, 1, 0, nullptr), n, "null");
  REFUSED(sr_add_gaussian_noise_f32(P, nullptr, nullptr, P, nullptr, Q, 1, 3, 8, 8, 1, 0, nullptr), n, "null");
  REFUSED(sr_add_gaussian_noise_f32(P, P, nullptr, nullptr, nullptr, Q, 1, 3, 8, 8, 1, 0, nullptr), n, "null");
  REFUSED(sr_add_gaussian_noise_f32(P, P, nullptr, P, nullptr, nullptr, 1, 3, 8, 8, 1, 0, nullptr), n, "null");
  REFUSED(sr_add_gaussian_noise_f32(P, P, nullptr, P, P, Q, 1, 3, 8, 8, 1, 0, nullptr), n, "gray needs noise_gray");
  REFUSED(sr_add_gaussian_noise_f32(P, P, nullptr, P, nullptr, Q, 0, 3, 8, 8, 1, 0, nullptr), n, "bad shape");
  REFUSED(sr_add_gaussian_noise_f32(P, P, nullptr, P, nullptr, Q, 1, 3, 8, 0, 1, 0, nullptr), n, "bad shape");
  REFUSED(sr_add_gaussian_noise_f32(P, P, nullptr, P, nullptr, Q, 1, -3, 8, 8, 1, 0, nullptr), n, "bad shape");

  const char* j = "sr_diffjpeg_f32";
  REFUSED(sr_diffjpeg_f32(nullptr, nullptr, P, Q, 1, 16, 16, 0, nullptr), j, "null");
  REFUSED(sr_diffjpeg_f32(P, S, nullptr, Q, 1, 16, 16, 0, nullptr), j, "null");
  REFUSED(sr_diffjpeg_f32(P, S, P, nullptr, 1, 16, 16, 1, nullptr), j, "null");
  REFUSED(sr_diffjpeg_f32(P, nullptr, P, Q, 0, 16, 16, 0, nullptr), j, "bad shape");
  REFUSED(sr_diffjpeg_f32(P, nullptr, P, Q, 1, 0, 16, 0, nullptr), j, "bad shape");
  REFUSED(sr_diffjpeg_f32(P, nullptr, P, Q, 1, 16, -16, 0, nullptr), j, "bad shape");
  REFUSED(sr_diffjpeg_f32(P, nullptr, P, Q, 1 << 15, 16, 16, 0, nullptr), j, "bad shape");

  const char* jb = "sr_diffjpeg_bwd_f32";
  REFUSED(sr_diffjpeg_bwd_f32(nullptr, nullptr, P, P, Q, 1, 16, 16, nullptr), jb, "null");
  REFUSED(sr_diffjpeg_bwd_f32(P, nullptr, nullptr, P, Q, 1, 16, 16, nullptr), jb, "null");
  REFUSED(sr_diffjpeg_bwd_f32(P, nullptr, P, nullptr, Q, 1, 16, 16, nullptr), jb, "null");
  REFUSED(sr_diffjpeg_bwd_f32(P, nullptr, P, P, nullptr, 1, 16, 16, nullptr), jb, "null");
  REFUSED(sr_diffjpeg_bwd_f32(P, nullptr, P, Q, Q, 0, 16, 16, nullptr), jb, "bad shape");
  REFUSED(sr_diffjpeg_bwd_f32(P, nullptr, P, Q, Q, 1, 16, 0, nullptr), jb, "bad shape");
  REFUSED(sr_diffjpeg_bwd_f32(P, nullptr, P, Q, P, 1, 16, 16, nullptr), jb, "must not be x");

  const char* e = "sr_degrade_finish_f32";
  const float m3[3] = {0.5f, 0.5f, 0.5f};
  REFUSED(sr_degrade_finish_f32(nullptr, nullptr, nullptr, Q, 1, 8, 8, m3, m3, nullptr), e, "null");
  REFUSED(sr_degrade_finish_f32(P, P, P, nullptr, 1, 8, 8, nullptr, nullptr, nullptr), e, "null");
  REFUSED(sr_degrade_finish_f32(P, nullptr, nullptr, Q, 0, 8, 8, m3, nullptr, nullptr), e, "bad shape");
  REFUSED(sr_degrade_finish_f32(P, nullptr, nullptr, Q, 1, 0, 8, nullptr, m3, nullptr), e, "bad shape");
  REFUSED(sr_degrade_finish_f32(P, nullptr, nullptr, Q, 1, 8, -8, nullptr, nullptr, nullptr), e, "bad shape");

  printf("degrade_host_checks: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
