// Host half of csrc/ema.hip without a GPU: the argument checks of vcg_ema_update and vcg_swap and the paths that return before a
// launch (n == 0, w == 0), as a stand-alone program for the host sanitizers.  It links ema.hip alone and supplies the one symbol
// that file takes from misc.hip (vcg_set_error).  No call below reaches a launch.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         tools/ema_host_check.cpp vae-cyclegan-implementation_amd/csrc/ema.hip -o tools/_build/ema_host_check
//   tools/_build/ema_host_check          (prints "ema_host_check: ok", exit status 0)
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/vcg.h"

static char g_err[256];
void vcg_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

static int failures = 0;
static void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "ema_host_check: FAILED: %s (last error: %s)\n", what, g_err);
    ++failures;
  }
}
static bool refused(int rc, const char* needle) { return rc != 0 && strstr(g_err, needle) != nullptr; }

int main() {
  // host memory: nothing below is launched on it
  float* buf = static_cast<float*>(aligned_alloc(64, 256 * sizeof(float)));
  for (int i = 0; i < 256; ++i) buf[i] = (float)i;
  float* a = buf;
  float* b = buf + 64;

  expect(refused(vcg_ema_update(nullptr, b, 8, 0.5f, nullptr, nullptr), "null pointer"), "ema_update: null e");
  expect(refused(vcg_ema_update(a, nullptr, 8, 0.5f, nullptr, nullptr), "null pointer"), "ema_update: null p");
  const float bad_w[] = {1.5f, -0.25f, NAN, INFINITY, -INFINITY, nextafterf(1.f, 2.f), -1e-45f};
  for (float w : bad_w) expect(refused(vcg_ema_update(a, b, 8, w, nullptr, nullptr), "[0, 1]"), "ema_update: w outside [0, 1]");
  expect(refused(vcg_ema_update(a + 1, b, 8, 0.5f, nullptr, nullptr), "aligned"), "ema_update: misaligned e");
  expect(refused(vcg_ema_update(a, b + 3, 8, 0.5f, nullptr, nullptr), "aligned"), "ema_update: misaligned p");
  expect(refused(vcg_ema_update(a, b, ((size_t)1 << 40) + 1, 0.5f, nullptr, nullptr), "too large"), "ema_update: n too large");
  expect(vcg_ema_update(a, b, 0, 0.5f, nullptr, nullptr) == 0, "ema_update: n == 0 is a no-op");
  expect(vcg_ema_update(a, b, 64, 0.f, nullptr, nullptr) == 0, "ema_update: w == 0 is a no-op");
  expect(vcg_ema_update(a, b, 64, -0.f, nullptr, nullptr) == 0, "ema_update: w == -0 is a no-op");

  expect(refused(vcg_swap(nullptr, b, 8, nullptr), "null pointer"), "swap: null a");
  expect(refused(vcg_swap(a, nullptr, 8, nullptr), "null pointer"), "swap: null b");
  expect(refused(vcg_swap(a, b + 1, 8, nullptr), "aligned"), "swap: misaligned b");
  expect(refused(vcg_swap(a + 2, b, 8, nullptr), "aligned"), "swap: misaligned a");
  expect(refused(vcg_swap(a, a, 8, nullptr), "overlap"), "swap: the same range");
  expect(refused(vcg_swap(a, a + 4, 8, nullptr), "overlap"), "swap: b inside a");
  expect(refused(vcg_swap(a + 4, a, 8, nullptr), "overlap"), "swap: a inside b");
  expect(refused(vcg_swap(a, a + 60, 64, nullptr), "overlap"), "swap: ranges sharing their last / first words");
  expect(refused(vcg_swap(a, b, ((size_t)1 << 40) + 1, nullptr), "too large"), "swap: n too large");
  expect(vcg_swap(a, a, 0, nullptr) == 0, "swap: n == 0 is a no-op");
  expect(vcg_swap(a, b, 0, nullptr) == 0, "swap: n == 0 is a no-op");

  for (int i = 0; i < 256; ++i) expect(buf[i] == (float)i, "a refused or empty call wrote to its arguments");
  free(buf);
  if (failures) return 1;
  puts("ema_host_check: ok");
  return 0;
}
