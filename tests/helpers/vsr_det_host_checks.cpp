// Stand-alone driver for the host-side code of vsr_det_ops.hip (include/sr_hip_vsr_det.h): the argument checks of the deterministic
// step-input adjoint and its workspace formula, run with the host sanitizers on a machine without a GPU.  Every call below returns
// before anything is launched.  The library services that translation unit uses are stubbed here.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       image_restoration_amd/csrc/vsr_det_ops.hip tests/helpers/vsr_det_host_checks.cpp \
//       -o vsr_det_host_checks && ./vsr_det_host_checks
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../image_restoration_amd/csrc/sr_internal.h"
#include "../../include/sr_hip_vsr_det.h"

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
// the call must be refused with `code` and a message that names the entry point and contains `needle`
#define REFUSED_AS(call, code, needle)                                                                              \
  do {                                                                                                              \
    g_err[0] = 0;                                                                                                   \
    ++checks;                                                                                                       \
    const int rc__ = (call);                                                                                        \
    if (rc__ != (code) || !strstr(g_err, "sr_vsr_prop_input_bwd_det_f32") || !strstr(g_err, needle)) {              \
      printf("FAILED line %d: %s -> %d (last error: %s)\n", __LINE__, #call, rc__, g_err);                          \
      ++failures;                                                                                                   \
    }                                                                                                               \
  } while (0)
#define REFUSED(call, needle) REFUSED_AS(call, SR_EINVAL, needle)
#define EXPECT(cond)                                    \
  do {                                                  \
    ++checks;                                           \
    if (!(cond)) {                                      \
      printf("FAILED line %d: %s\n", __LINE__, #cond);  \
      ++failures;                                       \
    }                                                   \
  } while (0)

static float* const G = (float*)256;
static float* const PREV = (float*)4096;
static float* const FLOW = (float*)8196;   // 4-byte aligned only
static float* const DPREV = (float*)12288;
static float* const DFLOW = (float*)16388;
static void* const WS = (void*)(uintptr_t)(1 << 20);

static sr_vsr_prop_bwd_det_desc good(int n = 2) {
  sr_vsr_prop_bwd_det_desc dd = {};
  sr_vsr_prop_bwd_desc& d = dd.d;
  d.g = G;
  d.prev = PREV;
  d.flow = FLOW;
  d.dprev = DPREV;
  d.dflow = DFLOW;
  d.g_img_stride = d.prev_img_stride = d.dprev_img_stride = 8 * 2 * 20;
  d.flow_img_stride = d.dflow_img_stride = 2 * 20;
  d.n = n;
  d.h = 4;
  d.w = 5;
  d.fb = 2;
  dd.workspace = WS;
  dd.workspace_bytes = sr_vsr_prop_input_bwd_det_workspace_bytes(n, 4, 5, 2);
  return dd;
}

int main() {
  // ---- the workspace formula: the int64 accumulators and one scale word per image, each rounded up to 256 bytes
  EXPECT(sr_vsr_prop_input_bwd_det_workspace_bytes(1, 1, 1, 1) == 256 + 256);
  EXPECT(sr_vsr_prop_input_bwd_det_workspace_bytes(2, 4, 5, 2) == sr::align_up((size_t)64 * 2 * 2 * 20, 256) + 256);
  EXPECT(sr_vsr_prop_input_bwd_det_workspace_bytes(4, 64, 64, 8) == (size_t)64 * 4 * 8 * 4096 + 256);
  EXPECT(sr_vsr_prop_input_bwd_det_workspace_bytes(65, 3, 3, 1) == sr::align_up((size_t)64 * 65 * 9, 256) + 512);
  EXPECT(sr_vsr_prop_input_bwd_det_workspace_bytes(1024, 1024, 1024, 1024) == ((size_t)64 << 40) + 4096);   // 2^40 elements
  EXPECT(sr_vsr_prop_input_bwd_det_workspace_bytes(65535, 16383, 16384, 65534) == 0);   // past 2^50 elements: refused, never wrapped
  const int bad[][4] = {{0, 4, 4, 1}, {65536, 4, 4, 1}, {1, 0, 4, 1}, {1, 4, -1, 1}, {1, 4, 4, 0}, {1, 4, 4, 65535}, {1, 16384, 16384, 1}};
  for (const auto& b : bad) EXPECT(sr_vsr_prop_input_bwd_det_workspace_bytes(b[0], b[1], b[2], b[3]) == 0);

  // ---- refusals, each before any launch
  REFUSED(sr_vsr_prop_input_bwd_det_f32(nullptr, nullptr), "null descriptor");
  sr_vsr_prop_bwd_det_desc dd = good();
  dd.d.g = nullptr;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "null g");
  dd = good();
  dd.d.prev = nullptr;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "null g");
  dd = good();
  dd.d.flow = nullptr;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "null g");
  dd = good();
  dd.d.dprev = nullptr;
  dd.d.dflow = nullptr;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "nothing to compute");
  for (int which = 0; which < 6; ++which) {
    dd = good();
    (which == 0 ? dd.d.n : which == 1 ? dd.d.h : which == 2 ? dd.d.w : dd.d.fb) = which < 4 ? 0 : which == 4 ? 65535 : -3;
    REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "bad shape");
  }
  dd = good();
  dd.d.n = 65536;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "bad shape");
  dd = good();
  dd.d.h = 1 << 14;
  dd.d.w = 1 << 14;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "too large");
  dd = good(1);
  dd.d.h = 1 << 13;
  dd.d.w = 1 << 13;
  dd.d.fb = 1 << 10;   // the window alone passes 2^38 floats
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "too large");
  dd = good();
  dd.d.g = (float*)260;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "16-byte aligned");
  dd = good();
  dd.d.dprev = (float*)12292;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "16-byte aligned");
  dd = good();
  dd.d.flow = (float*)8193;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "4-byte aligned");
  dd = good();
  dd.d.dflow = (float*)16386;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "4-byte aligned");
  dd = good();
  dd.d.prev_img_stride += 2;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "multiples of 4");
  dd = good();
  dd.d.dprev_img_stride += 1;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "multiples of 4");
  for (int which = 0; which < 5; ++which) {
    dd = good();
    (which == 0 ? dd.d.g_img_stride : which == 1 ? dd.d.prev_img_stride : which == 2 ? dd.d.dprev_img_stride
     : which == 3 ? dd.d.flow_img_stride : dd.d.dflow_img_stride) -= 4;
    REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "smaller than the image");
  }
  dd = good();
  dd.d.dprev = G;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "must not be a source");
  dd = good();
  dd.d.dprev = PREV;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "must not be a source");
  dd = good();
  dd.d.dflow = FLOW;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "must not be a source");
  // the workspace, needed with dprev only
  dd = good();
  dd.workspace = (char*)WS + 16;
  REFUSED(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), "256-byte aligned");
  dd = good();
  dd.workspace_bytes -= 1;
  REFUSED_AS(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), SR_ENOSPACE, "workspace");
  dd = good();
  dd.workspace = nullptr;
  REFUSED_AS(sr_vsr_prop_input_bwd_det_f32(&dd, nullptr), SR_ENOSPACE, "workspace of 0 bytes");
  printf("vsr_det_host_checks: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
