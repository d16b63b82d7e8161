// Stand-alone driver for the host-side code of dcn_ops_bf16.hip and edvr_ops_bf16.hip: the argument checks, the dispatch
// function and the pack size functions, built with the host sanitizers and run on a machine without a GPU.  Every call below
// returns before anything is launched.  The few library services those translation units use are stubbed here.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       image_restoration_amd/csrc/dcn_ops_bf16.hip image_restoration_amd/csrc/edvr_ops_bf16.hip \
//       tests/helpers/edvr_bf16_host_checks.cpp -o edvr_bf16_host_checks && ./edvr_bf16_host_checks
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../image_restoration_amd/csrc/sr_internal.h"
#include "../../include/sr_hip_edvr_bf16.h"

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

static sr_dcn_bf16_desc good() {
  sr_dcn_bf16_desc d;
  memset(&d, 0, sizeof d);
  void* p = (void*)256;
  d.x = p, d.offset = (const float*)p, d.mask = (const float*)p, d.wpacked = p, d.out = p;
  d.n = 1, d.cin = 64, d.cout = 64, d.h = 4, d.w = 4, d.deformable_groups = 8;
  d.x_img_stride = d.out_img_stride = 64 * 16, d.offset_img_stride = 144 * 16, d.mask_img_stride = 72 * 16;
  d.ksize = 3, d.stride = d.padding = d.dilation = d.groups = 1, d.act_slope = 1.f;
  return d;
}

int main() {
  sr_dcn_bf16_desc d = good();
  EXPECT(sr_dcn_fwd_bf16(nullptr, nullptr) == SR_EINVAL);
  d.cin = 48, d.deformable_groups = 4, d.x_img_stride = 48 * 16;
  EXPECT(sr_dcn_fwd_bf16(&d, nullptr) == SR_EINVAL && strstr(g_err, "multiple of 8"));
  d = good(), d.cin = 24, d.deformable_groups = 3;
  EXPECT(sr_dcn_fwd_bf16(&d, nullptr) == SR_EINVAL && strstr(g_err, "multiple of 16"));
  d = good(), d.ksize = 5;
  EXPECT(sr_dcn_fwd_bf16(&d, nullptr) == SR_EINVAL && strstr(g_err, "not supported"));
  d = good(), d.out = nullptr;
  EXPECT(sr_dcn_fwd_bf16(&d, nullptr) == SR_EINVAL && strstr(g_err, "null"));
  d = good(), d.x = (void*)264;
  EXPECT(sr_dcn_fwd_bf16(&d, nullptr) == SR_EINVAL && strstr(g_err, "aligned"));
  d = good(), d.mask_img_stride = 72 * 16 - 1;
  EXPECT(sr_dcn_fwd_bf16(&d, nullptr) == SR_EINVAL && strstr(g_err, "smaller than the image"));
  d = good(), d.h = 0;
  EXPECT(sr_dcn_fwd_bf16(&d, nullptr) == SR_EINVAL && strstr(g_err, "bad shape"));
  d = good(), d.h = 1 << 15, d.w = 1 << 15;  // strides checked in 64 bits, then the 32-bit plane offsets
  d.x_img_stride = d.out_img_stride = (int64_t)64 << 30, d.offset_img_stride = (int64_t)144 << 30, d.mask_img_stride = (int64_t)72 << 30;
  EXPECT(sr_dcn_fwd_bf16(&d, nullptr) == SR_EINVAL && strstr(g_err, "too large"));

  int cot = 0, rows = 0;
  EXPECT(sr_dcn_bf16_lds_bytes(64, 5, 180, 320, &cot, &rows) == 73728 && cot == 2 && rows == 4);
  EXPECT(sr_dcn_bf16_lds_bytes(24, 1, 9, 33, &cot, &rows) == 55296 && cot == 1 && rows == 4);
  EXPECT(sr_dcn_bf16_lds_bytes(64, 1, 1, 1, nullptr, nullptr) == 73728);
  EXPECT(sr_dcn_bf16_lds_bytes(0, 1, 1, 1, &cot, &rows) == 0 && sr_dcn_bf16_lds_bytes(64, 1, 0, 1, &cot, &rows) == 0);

  EXPECT(sr_conv1x1_packed_weight_elems_bf16(64, 320) == 64 * 320 && sr_conv1x1_packed_weight_elems_bf16(1, 16) == 32 * 16);
  EXPECT(sr_conv1x1_packed_weight_elems_bf16(16, 24) == 0 && sr_conv1x1_packed_weight_elems_bf16(-1, 16) == 0);
  EXPECT(sr_conv1x1_packed_weight_elems_bf16(1 << 20, 1 << 20) == ((size_t)1 << 40));
  void* p = (void*)256;
  EXPECT(sr_conv1x1_pack_bf16((const float*)p, nullptr, 16, 24, p, nullptr, nullptr) == SR_EINVAL);
  EXPECT(sr_conv1x1_pack_bf16((const float*)p, nullptr, 1 << 20, 1 << 20, p, nullptr, nullptr) == SR_EINVAL && strstr(g_err, "too large"));
  EXPECT(sr_conv1x1_bf16(p, 512, p, nullptr, p, 256, 1, 24, 16, 4, 4, 1.f, nullptr) == SR_EINVAL);
  EXPECT(sr_conv1x1_bf16(p, 504, p, nullptr, p, 256, 1, 32, 16, 4, 4, 1.f, nullptr) == SR_EINVAL && strstr(g_err, "stride"));
  EXPECT(sr_conv1x1_bf16(p, 512, p, (const float*)260, p, 256, 1, 32, 16, 4, 4, 1.f, nullptr) == SR_EINVAL && strstr(g_err, "aligned"));
  EXPECT(sr_conv1x1_bf16(p, (int64_t)1 << 40, p, nullptr, p, (int64_t)1 << 40, 1, 1 << 26, 16, 4, 4, 1.f, nullptr) == SR_EINVAL);
  EXPECT(sr_cb16_subsample2_bf16(p, 248, p, 64, 1, 1, 4, 4, nullptr) == SR_EINVAL);
  EXPECT(sr_cb16_subsample2_bf16(p, 256, p, 64, 1 << 30, 1 << 10, 1 << 15, 1 << 15, nullptr) == SR_EINVAL);
  EXPECT(sr_pool3x3s2_fwd_bf16(p, 256, p, 128, p, 56, 1, 1, 4, 4, nullptr) == SR_EINVAL);
  EXPECT(sr_tsa_corr_fwd_bf16(p, 384, p, 384, p, 384, nullptr, p, 384, 1, 1, 24, 4, 4, nullptr) == SR_EINVAL);
  EXPECT(sr_tsa_corr_fwd_bf16(p, 256, p, 256, p, 256, (float*)258, p, 256, 1, 1, 16, 4, 4, nullptr) == SR_EINVAL);
  EXPECT(sr_tsa_gate_fwd_bf16(p, 256, p, 256, p, 256, p, 248, 1, 1, 4, 4, nullptr) == SR_EINVAL);
  EXPECT(sr_tsa_gate_fwd_bf16(p, 256, p, 256, p, 256, p, 256, 1, 0, 4, 4, nullptr) == SR_EINVAL);
  if (failures)
    printf("%d checks failed\n", failures);
  else
    printf("all host checks passed\n");
  return failures ? 1 : 0;
}
