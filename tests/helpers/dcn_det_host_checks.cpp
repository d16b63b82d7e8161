// Stand-alone driver for the host-side code of dcn_det_ops.hip (include/sr_hip_dcn_det.h): the argument checks of the deterministic
// deformable-convolution input gradient and its workspace formula, run with the host sanitizers on a machine without a GPU.  Every
// call below returns before anything is launched.  dcn_ops.hip is linked in because the entry point takes the atomic entry point's
// own checks from it; the library services the two translation units use are stubbed here.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       image_restoration_amd/csrc/dcn_det_ops.hip image_restoration_amd/csrc/dcn_ops.hip tests/helpers/dcn_det_host_checks.cpp \
//       -o dcn_det_host_checks && ./dcn_det_host_checks
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../image_restoration_amd/csrc/sr_internal.h"
#include "../../include/sr_hip_dcn_det.h"

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
static int checks = 0;
// the call must be refused with `code` and a message that names `who` and contains `needle`
#define REFUSED_AS(call, code, who, needle)                                                  \
  do {                                                                                       \
    g_err[0] = 0;                                                                            \
    ++checks;                                                                                \
    const int rc__ = (call);                                                                 \
    if (rc__ != (code) || !strstr(g_err, who) || !strstr(g_err, needle)) {                   \
      printf("FAILED line %d: %s -> %d (last error: %s)\n", __LINE__, #call, rc__, g_err);   \
      ++failures;                                                                            \
    }                                                                                        \
  } while (0)
#define DET "sr_dcn_bwd_data_det_f32"
#define ATOMIC "sr_dcn_bwd_data_f32"   // the rules the entry point takes from the atomic one carry that one's name
#define REFUSED(call, needle) REFUSED_AS(call, SR_EINVAL, DET, needle)
#define REFUSED_BY_ATOMIC(call, needle) REFUSED_AS(call, SR_EINVAL, ATOMIC, needle)
#define EXPECT(cond)                                    \
  do {                                                  \
    ++checks;                                           \
    if (!(cond)) {                                      \
      printf("FAILED line %d: %s\n", __LINE__, #cond);  \
      ++failures;                                       \
    }                                                   \
  } while (0)

static float* at(uintptr_t mib, uintptr_t plus = 0) { return (float*)((mib << 20) + plus); }

static sr_dcn_bwd_det_desc good(int n = 2) {
  sr_dcn_bwd_det_desc dd = {};
  sr_dcn_bwd_desc& b = dd.d;
  sr_dcn_desc& f = b.fwd;
  const int h = 4, w = 5, cin = 16, dg = 2;
  f.x = at(1);
  f.offset = at(2);
  f.mask = at(3);
  f.x_img_stride = cin * h * w;
  f.offset_img_stride = 40 * h * w;   // 36 channels in 5 blocks
  f.mask_img_stride = 24 * h * w;     // 18 channels in 3 blocks
  f.n = n;
  f.cin = cin;
  f.cout = 8;
  f.h = h;
  f.w = w;
  f.deformable_groups = dg;
  f.ksize = 3;
  f.stride = f.padding = f.dilation = f.groups = 1;
  f.act_slope = 1.f;
  b.dcol = at(4);
  b.dx = at(5);
  b.doffset = at(6);
  b.dmask = at(7);
  b.dx_img_stride = f.x_img_stride;
  b.doffset_img_stride = f.offset_img_stride;
  b.dmask_img_stride = f.mask_img_stride;
  dd.workspace = at(8);
  dd.workspace_bytes = sr_dcn_bwd_data_det_workspace_bytes(n, cin, h, w);
  return dd;
}

int main() {
  // ---- the workspace formula: the int64 accumulators and two scale words per image, each rounded up to 256 bytes
  EXPECT(sr_dcn_bwd_data_det_workspace_bytes(1, 8, 1, 1) == 256 + 256);
  EXPECT(sr_dcn_bwd_data_det_workspace_bytes(2, 16, 4, 5) == sr::align_up((size_t)8 * 2 * 16 * 20, 256) + 256);
  EXPECT(sr_dcn_bwd_data_det_workspace_bytes(4, 64, 64, 64) == (size_t)8 * 4 * 64 * 4096 + 256);
  EXPECT(sr_dcn_bwd_data_det_workspace_bytes(33, 24, 3, 3) == sr::align_up((size_t)8 * 33 * 24 * 9, 256) + 512);
  EXPECT(sr_dcn_bwd_data_det_workspace_bytes(65535, 8, 1, 1) == sr::align_up((size_t)8 * 65535 * 8, 256) + sr::align_up((size_t)8 * 65535, 256));
  EXPECT(sr_dcn_bwd_data_det_workspace_bytes(65535, 64, 1024, 1820) == (size_t)8 * 65535 * 64 * 1024 * 1820 + sr::align_up((size_t)8 * 65535, 256));
  EXPECT(sr_dcn_bwd_data_det_workspace_bytes(1, 8 * 7281, 1, 1) != 0);
  const int bad[][4] = {{0, 8, 4, 4},       {65536, 8, 4, 4},  {1, 0, 4, 4},       {1, 12, 4, 4},      {1, -8, 4, 4},          {1, 8 * 7282, 1, 1},
                        {1, 8, 0, 4},       {1, 8, 4, -1},     {1, 8, 4096, 4096}, {1, 64, 1024, 2048}, {1, 8, 65536, 65536}, {1, 8, 2147483647, 2147483647}};
  for (const auto& b : bad) EXPECT(sr_dcn_bwd_data_det_workspace_bytes(b[0], b[1], b[2], b[3]) == 0);

  // ---- refusals, each before any launch
  REFUSED(sr_dcn_bwd_data_det_f32(nullptr, nullptr), "null descriptor");
  sr_dcn_bwd_det_desc dd = good();
  dd.d.fwd.x = nullptr;
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "null x");
  dd = good();
  dd.d.fwd.offset = nullptr;
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "null x");
  dd = good();
  dd.d.fwd.mask = nullptr;
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "null x");
  for (int which = 0; which < 5; ++which) {
    dd = good();
    (which == 0 ? dd.d.fwd.n : which == 1 ? dd.d.fwd.h : which == 2 ? dd.d.fwd.w : which == 3 ? dd.d.fwd.cin : dd.d.fwd.deformable_groups) =
        which == 1 ? -3 : 0;
    REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "bad shape");
  }
  dd = good();
  dd.d.fwd.cin = 12;
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "multiple of 8");
  dd = good();
  dd.d.fwd.deformable_groups = 4;
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "multiple of 8");
  for (int which = 0; which < 5; ++which) {
    dd = good();
    (which == 0 ? dd.d.fwd.ksize : which == 1 ? dd.d.fwd.stride : which == 2 ? dd.d.fwd.padding : which == 3 ? dd.d.fwd.dilation
                                                                                                             : dd.d.fwd.groups) += 1;
    REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "not supported");
  }
  dd = good();
  dd.d.fwd.x = at(1, 4);
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "16-byte aligned");
  dd = good();
  dd.d.fwd.mask_img_stride += 2;
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "16-byte aligned");
  dd = good();
  dd.d.fwd.h = dd.d.fwd.w = 1 << 14;
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "too large");
  dd = good();
  dd.d.dcol = nullptr;
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "null dcol");
  dd = good();
  dd.d.dcol = at(4, 8);
  REFUSED_BY_ATOMIC(sr_dcn_bwd_data_det_f32(&dd, nullptr), "16-byte aligned");
  // the destinations
  dd = good();
  dd.d.dmask = nullptr;
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "go together");
  dd = good();
  dd.d.doffset = nullptr;
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "go together");
  dd = good();
  dd.d.dx = at(5, 4);
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "16-byte aligned");
  dd = good();
  dd.d.doffset = at(6, 8);
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "16-byte aligned");
  dd = good();
  dd.d.dmask = at(7, 12);
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "16-byte aligned");
  dd = good();
  dd.d.dx_img_stride += 2;
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "multiple of 4");
  dd = good();
  dd.d.dx_img_stride -= 4;
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "smaller than the image");
  dd = good();
  dd.d.dx = at(1);
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "must not be a source");
  dd = good();
  dd.d.dx = at(4);
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "must not be a source");
  dd = good();
  dd.d.fwd.n = 65536;
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "bad shape");
  // the workspace, needed with dx only
  dd = good();
  dd.workspace = (char*)dd.workspace + 16;
  REFUSED(sr_dcn_bwd_data_det_f32(&dd, nullptr), "256-byte aligned");
  dd = good();
  dd.workspace_bytes -= 1;
  REFUSED_AS(sr_dcn_bwd_data_det_f32(&dd, nullptr), SR_ENOSPACE, DET, "sr_dcn_bwd_data_det_workspace_bytes");
  dd = good();
  dd.workspace = nullptr;
  REFUSED_AS(sr_dcn_bwd_data_det_f32(&dd, nullptr), SR_ENOSPACE, DET, "workspace of 0 bytes");
  // nothing asked for is nothing done, without a workspace
  dd = good();
  dd.d.dx = dd.d.doffset = dd.d.dmask = nullptr;
  dd.workspace = nullptr;
  dd.workspace_bytes = 0;
  EXPECT(sr_dcn_bwd_data_det_f32(&dd, nullptr) == SR_OK);
  printf("dcn_det_host_checks: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
