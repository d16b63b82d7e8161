// Stand-alone driver for the host-side code of flow_ops.hip: the argument checks, the dispatch (sr_conv7x7_instance) and the size
// queries of its entry points, built with the host sanitizers and run on a machine without a GPU.  Every call below returns
// before anything is launched.  The few library services that translation unit uses are stubbed here.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       image_restoration_amd/csrc/flow_ops.hip tests/helpers/flow_host_checks.cpp \
//       -o flow_host_checks && ./flow_host_checks
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../image_restoration_amd/csrc/sr_internal.h"
#include "../../include/sr_hip_flow.h"

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

static float* const P = (float*)256;
static float* const Q = (float*)4096;
static float* const ODD = (float*)260;  // 4-byte aligned only

static sr_conv7x7_desc good() {
  sr_conv7x7_desc d = {};
  d.in = P;
  d.in_img_stride = 8 * 16 * 16;
  d.cin = 8;
  d.cout = 32;
  d.n = 1;
  d.h = 16;
  d.w = 16;
  d.packed = Q;
  d.out = Q;
  d.out_img_stride = 32 * 16 * 16;
  return d;
}

int main() {
  // dispatch and size queries
  const int shapes[5][3] = {{8, 32, 0}, {32, 64, 1}, {64, 32, 0}, {32, 16, 0}, {16, 2, 2}};
  for (const auto& s : shapes) EXPECT(sr_conv7x7_instance(s[1], s[0]) == s[2]);
  EXPECT(sr_conv7x7_packed_floats(32, 8) == 49u * 32 * 8 + 32);
  EXPECT(sr_conv7x7_packed_floats(64, 32) == 49u * 64 * 32 + 64);
  EXPECT(sr_conv7x7_packed_floats(32, 64) == 49u * 32 * 64 + 32);
  EXPECT(sr_conv7x7_packed_floats(16, 32) == 49u * 32 * 32 + 32);  // 16 couts padded to 32
  EXPECT(sr_conv7x7_packed_floats(2, 16) == 49u * 4 * 16 + 32);    // 2 couts padded to 4
  for (int cin = -8; cin <= 72; ++cin)
    for (int cout = -2; cout <= 70; ++cout) {
      bool served = false;
      for (const auto& s : shapes) served = served || (s[0] == cin && s[1] == cout);
      if (!served) {
        EXPECT(sr_conv7x7_instance(cout, cin) == -1);
        EXPECT(sr_conv7x7_packed_floats(cout, cin) == 0);
      }
    }

  const char* pk = "sr_conv7x7_pack_f32";
  REFUSED(sr_conv7x7_pack_f32(P, P, 32, 16, Q, nullptr), pk, "not supported");
  REFUSED(sr_conv7x7_pack_f32(P, P, 3, 8, Q, nullptr), pk, "not supported");
  REFUSED(sr_conv7x7_pack_f32(nullptr, P, 32, 8, Q, nullptr), pk, "null");
  REFUSED(sr_conv7x7_pack_f32(P, nullptr, 32, 8, nullptr, nullptr), pk, "null");
  REFUSED(sr_conv7x7_pack_f32(P, nullptr, 32, 8, ODD, nullptr), pk, "aligned");

  const char* c = "sr_conv7x7_f32";
  sr_conv7x7_desc d;
  REFUSED(sr_conv7x7_f32(nullptr, nullptr), c, "null descriptor");
  d = good(), d.cin = 16;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "not supported");
  d = good(), d.cout = 2;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "not supported");
  d = good(), d.in = nullptr;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "null");
  d = good(), d.packed = nullptr;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "null");
  d = good(), d.out = nullptr;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "null");
  d = good(), d.n = 0;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "bad shape");
  d = good(), d.h = -1;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "bad shape");
  d = good(), d.w = 0;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "bad shape");
  d = good(), d.in = ODD;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "aligned");
  d = good(), d.res1 = ODD;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "aligned");
  d = good(), d.out_img_stride += 2;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "multiples of 4");
  d = good(), d.relu = 2;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "relu");
  d = good(), d.h = 8192, d.w = 8192, d.in_img_stride = d.out_img_stride = 1ll << 40;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "too large");
  d = good(), d.in_img_stride = 8;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "smaller than the image");
  d = good(), d.res1 = P, d.res1_img_stride = 0;
  REFUSED(sr_conv7x7_f32(&d, nullptr), c, "smaller than the image");

  const char* w = "sr_flow_warp_f32";
  REFUSED(sr_flow_warp_f32(nullptr, P, Q, 1, 3, 8, 8, 0, 0, nullptr), w, "null");
  REFUSED(sr_flow_warp_f32(P, nullptr, Q, 1, 3, 8, 8, 0, 0, nullptr), w, "null");
  REFUSED(sr_flow_warp_f32(P, P, nullptr, 1, 3, 8, 8, 0, 0, nullptr), w, "null");
  REFUSED(sr_flow_warp_f32(P, P, Q, 0, 3, 8, 8, 0, 0, nullptr), w, "bad shape");
  REFUSED(sr_flow_warp_f32(P, P, Q, 1, 0, 8, 8, 0, 0, nullptr), w, "bad shape");
  REFUSED(sr_flow_warp_f32(P, P, Q, 1, 3, -8, 8, 0, 0, nullptr), w, "bad shape");
  REFUSED(sr_flow_warp_f32(P, P, Q, 1, 3, 8, 0, 0, 0, nullptr), w, "bad shape");
  REFUSED(sr_flow_warp_f32(P, P, Q, 1, 3, 8, 8, 2, 0, nullptr), w, "layout");
  REFUSED(sr_flow_warp_f32(P, P, Q, 1, 3, 8, 8, -1, 0, nullptr), w, "layout");
  REFUSED(sr_flow_warp_f32(P, P, Q, 1, 3, 8, 8, 0, 2, nullptr), w, "padding");  // reflection is not served
  REFUSED(sr_flow_warp_f32(P, P, Q, 1, 3, 1 << 15, 1 << 15, 0, 0, nullptr), w, "too large");
  REFUSED(sr_flow_warp_f32(P, P, Q, 1 << 16, 3, 8, 8, 0, 0, nullptr), w, "grid");
  REFUSED(sr_flow_warp_f32(P, ODD, Q, 1, 3, 8, 8, 0, 0, nullptr), w, "8-byte");
  REFUSED(sr_flow_warp_f32(ODD, P, Q, 1, 3, 8, 8, 1, 0, nullptr), w, "16-byte");
  REFUSED(sr_flow_warp_f32(P, P, ODD, 1, 3, 8, 8, 1, 0, nullptr), w, "16-byte");

  const char* b = "sr_flow_warp_bwd_f32";
  REFUSED(sr_flow_warp_bwd_f32(nullptr, P, P, Q, Q, 1, 3, 8, 8, 0, 0, nullptr), b, "null");
  REFUSED(sr_flow_warp_bwd_f32(P, P, nullptr, Q, Q, 1, 3, 8, 8, 0, 0, nullptr), b, "null g");
  REFUSED(sr_flow_warp_bwd_f32(P, P, P, Q, Q, 1, 3, 8, 8, 0, 3, nullptr), b, "padding");
  REFUSED(sr_flow_warp_bwd_f32(P, P, P, Q, Q, 1, 3, 8, 8, 5, 0, nullptr), b, "layout");
  REFUSED(sr_flow_warp_bwd_f32(P, P, P, Q, ODD, 1, 3, 8, 8, 0, 0, nullptr), b, "8-byte");
  ++checks;  // neither gradient wanted: nothing to launch, SR_OK
  if (sr_flow_warp_bwd_f32(P, P, P, nullptr, nullptr, 1, 3, 8, 8, 0, 0, nullptr) != SR_OK) {
    printf("FAILED line %d: a call that wants no gradient must return SR_OK\n", __LINE__);
    ++failures;
  }

  const char* l = "sr_spynet_level_input_f32";
  REFUSED(sr_spynet_level_input_f32(nullptr, P, nullptr, Q, Q, 1, 8, 8, nullptr), l, "null");
  REFUSED(sr_spynet_level_input_f32(P, P, nullptr, nullptr, Q, 1, 8, 8, nullptr), l, "null");
  REFUSED(sr_spynet_level_input_f32(P, P, nullptr, Q, nullptr, 1, 8, 8, nullptr), l, "null");
  REFUSED(sr_spynet_level_input_f32(P, P, nullptr, Q, Q, 0, 8, 8, nullptr), l, "bad shape");
  REFUSED(sr_spynet_level_input_f32(P, P, nullptr, Q, Q, 1, 0, 8, nullptr), l, "bad shape");
  REFUSED(sr_spynet_level_input_f32(P, P, P, Q, Q, 1, 7, 8, nullptr), l, "even");
  REFUSED(sr_spynet_level_input_f32(P, P, P, Q, Q, 1, 8, 9, nullptr), l, "even");
  REFUSED(sr_spynet_level_input_f32(P, P, nullptr, ODD, Q, 1, 8, 8, nullptr), l, "aligned");
  REFUSED(sr_spynet_level_input_f32(P, P, ODD, Q, Q, 1, 8, 8, nullptr), l, "aligned");

  const char* n = "sr_spynet_preprocess_f32";
  const float m3[3] = {0.5f, 0.5f, 0.5f}, z3[3] = {0.5f, 0.f, 0.5f};
  REFUSED(sr_spynet_preprocess_f32(nullptr, Q, 1, 8, 8, m3, m3, nullptr), n, "null");
  REFUSED(sr_spynet_preprocess_f32(P, Q, 1, 8, 8, nullptr, m3, nullptr), n, "null");
  REFUSED(sr_spynet_preprocess_f32(P, Q, 1, 8, 8, m3, nullptr, nullptr), n, "null");
  REFUSED(sr_spynet_preprocess_f32(P, Q, 0, 8, 8, m3, m3, nullptr), n, "bad shape");
  REFUSED(sr_spynet_preprocess_f32(P, Q, 1, 8, -8, m3, m3, nullptr), n, "bad shape");
  REFUSED(sr_spynet_preprocess_f32(P, Q, 1, 8, 8, m3, z3, nullptr), n, "std3[1]");

  const char* a = "sr_avgpool2x2_f32";
  REFUSED(sr_avgpool2x2_f32(nullptr, Q, 3, 8, 8, nullptr), a, "null");
  REFUSED(sr_avgpool2x2_f32(P, nullptr, 3, 8, 8, nullptr), a, "null");
  REFUSED(sr_avgpool2x2_f32(P, Q, 0, 8, 8, nullptr), a, "even");
  REFUSED(sr_avgpool2x2_f32(P, Q, 3, 7, 8, nullptr), a, "even");
  REFUSED(sr_avgpool2x2_f32(P, Q, 3, 8, 0, nullptr), a, "even");
  REFUSED(sr_avgpool2x2_f32(P, Q, 1 << 16, 8, 8, nullptr), a, "planes");
  REFUSED(sr_avgpool2x2_f32(ODD, Q, 3, 8, 8, nullptr), a, "8-byte");

  printf("flow_host_checks: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
