// Stand-alone driver for the host-side code of adam_groups.hip: the argument checks and the class table the kernel receives by
// value, built with the host sanitizers and run on a machine without a GPU.  Every call below returns before anything is
// launched.  The few library services that translation unit uses are stubbed here.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       image_restoration_amd/csrc/adam_groups.hip tests/helpers/adam_groups_host_checks.cpp \
//       -o adam_groups_host_checks && ./adam_groups_host_checks
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../image_restoration_amd/csrc/sr_internal.h"
#include "../../include/sr_hip_train_groups.h"

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
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static float* const P = (float*)256;
static const uint8_t* const CLS = (const uint8_t*)4096;

static int step(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* cls, const sr_adam_class* classes, int nc) {
  g_err[0] = 0;
  return sr_adam_step_groups_f32(p, g, m, v, n, cls, classes, nc, 0.9f, 0.99f, 1e-8f, 0.f, 1.f, nullptr, nullptr, nullptr);
}

int main() {
  sr_adam_class one[1] = {{1e-4f, 1, 1}};
  // every refusal comes before the launch
  EXPECT(step(nullptr, P, P, P, 64, CLS, one, 1) == SR_EINVAL && strstr(g_err, "null"));
  EXPECT(step(P, nullptr, P, P, 64, CLS, one, 1) == SR_EINVAL && step(P, P, nullptr, P, 64, CLS, one, 1) == SR_EINVAL);
  EXPECT(step(P, P, P, nullptr, 64, CLS, one, 1) == SR_EINVAL && step(P, P, P, P, 64, nullptr, one, 1) == SR_EINVAL);
  EXPECT(step(P, P, P, P, 64, CLS, nullptr, 1) == SR_EINVAL && strstr(g_err, "null classes"));
  EXPECT(step((float*)260, P, P, P, 64, CLS, one, 1) == SR_EINVAL && strstr(g_err, "aligned"));
  EXPECT(step(P, P, P, (float*)264, 64, CLS, one, 1) == SR_EINVAL && strstr(g_err, "aligned"));
  EXPECT(step(P, P, P, P, 0, CLS, one, 1) == SR_EINVAL && strstr(g_err, "multiple of 64"));
  EXPECT(step(P, P, P, P, -64, CLS, one, 1) == SR_EINVAL && step(P, P, P, P, 100, CLS, one, 1) == SR_EINVAL);
  EXPECT(step(P, P, P, P, (int64_t)1 << 50, CLS, one, 1) == SR_EINVAL && strstr(g_err, "grid"));
  EXPECT(step(P, P, P, P, 64, CLS, one, 0) == SR_EINVAL && strstr(g_err, "outside 1..16"));
  EXPECT(step(P, P, P, P, 64, CLS, one, 17) == SR_EINVAL && step(P, P, P, P, 64, CLS, one, -1) == SR_EINVAL);
  sr_adam_class bad[3] = {{1e-4f, 4, 1}, {1e-4f, -2, 0}, {1e-4f, -2, 1}};
  float t4[4][3];
  int a3[3];
  EXPECT(sr_adam_class_table(bad, 2, 0.9f, 0.99f, t4[0], t4[1], t4[2], a3) == SR_OK && a3[1] == 0);   // an inactive class may carry any step
  EXPECT(step(P, P, P, P, 64, CLS, bad, 3) == SR_EINVAL && strstr(g_err, "class 2 has step -2"));

  // the class table: exactly n_classes entries are read and written, at the smallest and the largest table
  for (int nc : {1, 2, SR_ADAM_MAX_CLASSES}) {
    sr_adam_class* cl = new sr_adam_class[nc];
    float *lr = new float[nc], *bc1 = new float[nc], *bc2 = new float[nc];
    int* act = new int[nc];
    for (int c = 0; c < nc; ++c) cl[c] = {1e-4f * (c + 1), c % 3 == 2 ? -7 : 1 + 1000 * c, c % 3 != 2};
    g_err[0] = 0;
    EXPECT(sr_adam_class_table(cl, nc, 0.9f, 0.99f, lr, bc1, bc2, act) == SR_OK);
    for (int c = 0; c < nc; ++c) {
      if (c % 3 == 2) {
        EXPECT(act[c] == 0 && lr[c] == 0.f && bc1[c] == 1.f && bc2[c] == 1.f);
      } else {
        EXPECT(act[c] == 1 && lr[c] == cl[c].lr);
        EXPECT(bc1[c] == (float)(1.0 - pow((double)0.9f, cl[c].step)) && bc2[c] == (float)sqrt(1.0 - pow((double)0.99f, cl[c].step)));
      }
    }
    delete[] cl;
    delete[] lr;
    delete[] bc1;
    delete[] bc2;
    delete[] act;
  }
  float f[1];
  int a[1];
  EXPECT(sr_adam_class_table(one, 1, 0.9f, 0.99f, nullptr, f, f, a) == SR_EINVAL && strstr(g_err, "null output"));
  EXPECT(sr_adam_class_table(nullptr, 1, 0.9f, 0.99f, f, f, f, a) == SR_EINVAL && sr_adam_class_table(one, 17, 0.9f, 0.99f, f, f, f, a) == SR_EINVAL);
  one[0].step = 0;
  EXPECT(sr_adam_class_table(one, 1, 0.9f, 0.99f, f, f, f, a) == SR_EINVAL && strstr(g_err, "step 0 < 1"));
  if (failures)
    printf("%d checks failed\n", failures);
  else
    printf("all host checks passed\n");
  return failures ? 1 : 0;
}
