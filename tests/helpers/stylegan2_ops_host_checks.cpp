// Stand-alone driver for the host-side code of stylegan2_ops.hip: the argument checks, the dispatch function and the workspace
// size query, built with the host sanitizers and run on a machine without a GPU.  Every call below returns before anything is
// launched.  The few library services that translation unit uses are stubbed here.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       image_restoration_amd/csrc/stylegan2_ops.hip tests/helpers/stylegan2_ops_host_checks.cpp \
//       -o stylegan2_ops_host_checks && ./stylegan2_ops_host_checks
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../image_restoration_amd/csrc/sr_internal.h"
#include "../../include/sr_hip_stylegan2.h"

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
int ensure_dynamic_lds(const void*, int) { return SR_OK; }
}  // namespace sr

static int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static float* const P = (float*)256;

// sr_upfirdn2d_f32 on a 6x9 plane with one argument group replaced
static int ufd(int kh, int kw, int ux, int uy, int dx, int dy, int px0, int px1, int py0, int py1, int in_h = 6, int in_w = 9,
               int minor = 1, int n = 1, int planes = 1, int64_t xs = 1 << 20, int64_t os = 1 << 20) {
  g_err[0] = 0;
  return sr_upfirdn2d_f32(P, xs, P, os, P, n, planes, in_h, in_w, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1, nullptr);
}

int main() {
  // the dispatch: every instance, the tile rows the 63 KiB budget allows, the refusals
  int th = 0;
  size_t lds = 0;
  EXPECT(sr_upfirdn2d_instance(4, 4, 1, 1, 1, 1, &th, &lds) == 1 && th == 32 && lds == (256 + 35 * 67) * 4);
  EXPECT(sr_upfirdn2d_instance(4, 4, 2, 2, 1, 1, &th, &lds) == 2 && th == 32 && lds == (256 + 18 * 34) * 4);
  EXPECT(sr_upfirdn2d_instance(4, 4, 1, 1, 2, 2, &th, &lds) == 3 && th == 32 && lds == (256 + 66 * 130) * 4);
  EXPECT(sr_upfirdn2d_instance(4, 4, 2, 1, 1, 1, &th, &lds) == 0 && th == 32);   // mixed factors: generic
  EXPECT(sr_upfirdn2d_instance(4, 4, 2, 2, 2, 2, nullptr, nullptr) == 0);
  EXPECT(sr_upfirdn2d_instance(3, 4, 1, 1, 1, 1, nullptr, nullptr) == 0 && sr_upfirdn2d_instance(1, 1, 1, 1, 1, 1, &th, &lds) == 0);
  EXPECT(th == 32 && lds == (256 + 32 * 64) * 4);
  EXPECT(sr_upfirdn2d_instance(16, 16, 1, 1, 8, 8, &th, &lds) == 0 && th == 2 && lds == (256 + 24 * 520) * 4 && lds <= 63 * 1024);
  EXPECT(sr_upfirdn2d_instance(16, 16, 8, 8, 8, 8, &th, &lds) == 0 && th == 32 && lds <= 63 * 1024);
  EXPECT(sr_upfirdn2d_instance(16, 16, 1, 8, 8, 1, &th, &lds) == 0 && lds <= 63 * 1024);
  for (int kh = 1; kh <= 16; ++kh)
    for (int u = 1; u <= 8; ++u)
      for (int d = 1; d <= 8; ++d) {
        EXPECT(sr_upfirdn2d_instance(kh, 17 - kh, u, 9 - u, d, 9 - d, &th, &lds) == 0 && th >= 1 && lds <= 63 * 1024);
        EXPECT(sr_upfirdn2d_instance(kh, kh, u, u, d, d, &th, &lds) >= 0 && th >= 1 && lds <= 63 * 1024);
      }
  EXPECT(sr_upfirdn2d_instance(0, 4, 1, 1, 1, 1, &th, &lds) == -1 && sr_upfirdn2d_instance(4, 17, 1, 1, 1, 1, &th, &lds) == -1);
  EXPECT(sr_upfirdn2d_instance(4, 4, 0, 1, 1, 1, &th, &lds) == -1 && sr_upfirdn2d_instance(4, 4, 1, 9, 1, 1, &th, &lds) == -1);
  EXPECT(sr_upfirdn2d_instance(4, 4, 1, 1, 9, 1, &th, &lds) == -1 && sr_upfirdn2d_instance(4, 4, 1, 1, 1, 0, &th, &lds) == -1);

  // sr_upfirdn2d_f32: every refusal comes before the launch
  EXPECT(sr_upfirdn2d_f32(nullptr, 54, P, 54, P, 1, 1, 6, 9, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, nullptr) == SR_EINVAL && strstr(g_err, "null"));
  EXPECT(sr_upfirdn2d_f32(P, 54, nullptr, 54, P, 1, 1, 6, 9, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, nullptr) == SR_EINVAL);
  EXPECT(sr_upfirdn2d_f32(P, 54, P, 54, nullptr, 1, 1, 6, 9, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, nullptr) == SR_EINVAL);
  EXPECT(sr_upfirdn2d_f32((float*)258, 54, P, 54, P, 1, 1, 6, 9, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, nullptr) == SR_EINVAL && strstr(g_err, "aligned"));
  EXPECT(ufd(4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 6, 9, 2) == SR_EINVAL && strstr(g_err, "minor"));
  EXPECT(ufd(4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 0, 9) == SR_EINVAL && strstr(g_err, "bad shape"));
  EXPECT(ufd(4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 6, 9, 1, 0) == SR_EINVAL && ufd(4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 6, 9, 1, 1, 0) == SR_EINVAL);
  EXPECT(ufd(17, 4, 1, 1, 1, 1, 20, 0, 20, 0) == SR_EINVAL && strstr(g_err, "not supported"));
  EXPECT(ufd(4, 0, 1, 1, 1, 1, 0, 0, 0, 0) == SR_EINVAL && ufd(4, 4, 9, 1, 1, 1, 0, 0, 0, 0) == SR_EINVAL);
  EXPECT(ufd(4, 4, 1, 1, 1, 0, 0, 0, 0, 0) == SR_EINVAL && strstr(g_err, "not supported"));
  EXPECT(ufd(4, 4, 1, 1, 1, 1, -3, -3, 0, 0) == SR_EINVAL && strstr(g_err, "not positive"));     // 9 - 6 - 4 < 0
  EXPECT(ufd(7, 4, 1, 1, 1, 1, 0, 0, 0, 0) == SR_EINVAL && strstr(g_err, "not positive"));       // 6 - 7 < 0
  EXPECT(ufd(4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 6, 9, 1, 1, 2, 107) == SR_EINVAL && strstr(g_err, "stride"));
  EXPECT(ufd(4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 6, 9, 1, 1, 2, 108, 35) == SR_EINVAL && strstr(g_err, "stride"));
  EXPECT(ufd(4, 4, 8, 8, 1, 1, 0, 0, 0, 0, 1 << 27, 9) == SR_EINVAL && strstr(g_err, "2^30"));
  EXPECT(ufd(4, 4, 1, 1, 1, 1, 0x7fffffff, 0x7fffffff, 0, 0) == SR_EINVAL && strstr(g_err, "2^30"));
  EXPECT(ufd(4, 4, 1, 1, 1, 1, -0x7fffffff - 1, 0x7fffffff, 0, 0) == SR_EINVAL && strstr(g_err, "2^30"));
  EXPECT(ufd(1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 64, 64, 1, 1 << 16, 1 << 16, (int64_t)1 << 28, (int64_t)1 << 28) == SR_EINVAL && strstr(g_err, "grid"));
  EXPECT(ufd(1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1 << 14, 1 << 14, 1, 1 << 10, 1 << 10, (int64_t)1 << 38, (int64_t)1 << 38) == SR_EINVAL && strstr(g_err, "grid"));

  // the activation: refusals and the workspace size (the partials of the scalar pass)
  EXPECT(sr_fused_bias_act_f32(nullptr, P, nullptr, P, 1, 1, 1, 0.2f, 1.f, nullptr) == SR_EINVAL && strstr(g_err, "null"));
  EXPECT(sr_fused_bias_act_f32(P, P, nullptr, nullptr, 1, 1, 1, 0.2f, 1.f, nullptr) == SR_EINVAL);
  EXPECT(sr_fused_bias_act_f32(P, (float*)257, nullptr, P, 1, 1, 1, 0.2f, 1.f, nullptr) == SR_EINVAL && strstr(g_err, "aligned"));
  EXPECT(sr_fused_bias_act_f32(P, P, nullptr, P, 0, 1, 1, 0.2f, 1.f, nullptr) == SR_EINVAL && strstr(g_err, "bad shape"));
  EXPECT(sr_fused_bias_act_f32(P, P, nullptr, P, 1, 0, 1, 0.2f, 1.f, nullptr) == SR_EINVAL);
  EXPECT(sr_fused_bias_act_f32(P, P, nullptr, P, 1, 1, 0, 0.2f, 1.f, nullptr) == SR_EINVAL);
  EXPECT(sr_fused_bias_act_f32(P, P, nullptr, P, 1 << 16, 1 << 16, 1, 0.2f, 1.f, nullptr) == SR_EINVAL && strstr(g_err, "grid"));
  EXPECT(sr_fused_bias_act_f32(P, P, nullptr, P, 1 << 10, 1 << 10, (int64_t)1 << 24, 0.2f, 1.f, nullptr) == SR_EINVAL && strstr(g_err, "grid"));
  EXPECT(sr_fused_bias_act_f32(P, P, nullptr, P, 1, 1, (int64_t)1 << 62, 0.2f, 1.f, nullptr) == SR_EINVAL && strstr(g_err, "grid"));
  EXPECT(sr_fused_bias_act_workspace_bytes(2, 3, 1) == 24 && sr_fused_bias_act_workspace_bytes(2, 3, 1024) == 24);
  EXPECT(sr_fused_bias_act_workspace_bytes(2, 3, 1025) == 48 && sr_fused_bias_act_workspace_bytes(16, 64, 256 * 256) == 16 * 64 * 64 * 4);
  EXPECT(sr_fused_bias_act_workspace_bytes(0, 3, 1) == 0 && sr_fused_bias_act_workspace_bytes(2, 3, 0) == 0);
  EXPECT(sr_fused_bias_act_workspace_bytes(1 << 16, 1 << 16, 1) == 0 && sr_fused_bias_act_workspace_bytes(1, 1, (int64_t)1 << 62) == 0);
  EXPECT(sr_fused_bias_act_bwd_f32(nullptr, P, P, P, 1, 1, 1, 0.2f, 1.f, P, 4, nullptr) == SR_EINVAL && strstr(g_err, "null"));
  EXPECT(sr_fused_bias_act_bwd_f32(P, nullptr, P, P, 1, 1, 1, 0.2f, 1.f, P, 4, nullptr) == SR_EINVAL);
  EXPECT(sr_fused_bias_act_bwd_f32(P, P, nullptr, P, 1, 1, 1, 0.2f, 1.f, P, 4, nullptr) == SR_EINVAL);
  EXPECT(sr_fused_bias_act_bwd_f32(P, P, P, (float*)258, 1, 1, 1, 0.2f, 1.f, P, 4, nullptr) == SR_EINVAL && strstr(g_err, "aligned"));
  EXPECT(sr_fused_bias_act_bwd_f32(P, P, P, P, 1, 0, 1, 0.2f, 1.f, P, 4, nullptr) == SR_EINVAL && strstr(g_err, "bad shape"));
  EXPECT(sr_fused_bias_act_bwd_f32(P, P, P, P, 1 << 16, 1 << 16, 1, 0.2f, 1.f, P, 4, nullptr) == SR_EINVAL && strstr(g_err, "grid"));
  EXPECT(sr_fused_bias_act_bwd_f32(P, P, P, P, 2, 3, 1025, 0.2f, 1.f, nullptr, 48, nullptr) == SR_EINVAL && strstr(g_err, "workspace"));
  EXPECT(sr_fused_bias_act_bwd_f32(P, P, P, P, 2, 3, 1025, 0.2f, 1.f, P, 47, nullptr) == SR_ENOSPACE && strstr(g_err, "48 needed"));
  if (failures)
    printf("%d checks failed\n", failures);
  else
    printf("all host checks passed\n");
  return failures ? 1 : 0;
}
