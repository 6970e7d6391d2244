// Host half of csrc/image_pool.hip without a GPU: the argument checks of vcg_pool_exchange and the path that returns before a
// launch (N == 0), as a stand-alone program for the host sanitizers.  It links image_pool.hip alone and supplies the one symbol that
// file takes from misc.hip (vcg_set_error).  No call below reaches a launch.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         tools/image_pool_host_check.cpp vae-cyclegan-implementation_amd/csrc/image_pool.hip -o tools/_build/image_pool_host_check
//   tools/_build/image_pool_host_check          (prints "image_pool_host_check: ok", exit status 0)
#include <limits.h>
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
    fprintf(stderr, "image_pool_host_check: FAILED: %s (last error: %s)\n", what, g_err);
    ++failures;
  }
}
static bool refused(int rc, const char* needle) { return rc != 0 && strstr(g_err, needle) != nullptr; }

int main() {
  // host memory: nothing below is launched on it.  fake | out | pool: 2 images, 2 images, 4 slots of 16 floats
  const int N = 2, cap = 4;
  const size_t elems = 16;
  float* buf = static_cast<float*>(aligned_alloc(64, 256 * sizeof(float)));
  for (int i = 0; i < 256; ++i) buf[i] = (float)i;
  float *fake = buf, *out = buf + 32, *pool = buf + 64;
  const int32_t ok[2] = {0, -3};

  expect(refused(vcg_pool_exchange(nullptr, pool, out, ok, N, elems, cap, nullptr), "null pointer"), "null fake");
  expect(refused(vcg_pool_exchange(fake, nullptr, out, ok, N, elems, cap, nullptr), "null pointer"), "null pool");
  expect(refused(vcg_pool_exchange(fake, pool, nullptr, ok, N, elems, cap, nullptr), "null pointer"), "null out");
  expect(refused(vcg_pool_exchange(fake, pool, out, nullptr, N, elems, cap, nullptr), "null pointer"), "null plan");
  expect(refused(vcg_pool_exchange(fake + 1, pool, out, ok, 1, elems, cap, nullptr), "aligned"), "misaligned fake");
  expect(refused(vcg_pool_exchange(fake, pool + 2, out, ok, N, elems, cap - 1, nullptr), "aligned"), "misaligned pool");
  expect(refused(vcg_pool_exchange(fake, pool, out + 3, ok, 1, elems, cap, nullptr), "aligned"), "misaligned out");
  expect(refused(vcg_pool_exchange(fake, pool, out, ok, -1, elems, cap, nullptr), "negative"), "N < 0");
  expect(refused(vcg_pool_exchange(fake, pool, out, ok, INT_MIN, elems, cap, nullptr), "negative"), "N = INT_MIN");
  expect(refused(vcg_pool_exchange(fake, pool, out, ok, N, elems, 0, nullptr), "capacity"), "capacity 0");
  expect(refused(vcg_pool_exchange(fake, pool, out, ok, N, elems, INT_MIN, nullptr), "capacity"), "capacity INT_MIN");
  expect(refused(vcg_pool_exchange(fake, pool, out, ok, N, 0, cap, nullptr), "elems == 0"), "elems == 0 with images");
  expect(refused(vcg_pool_exchange(fake, pool, out, ok, N, ((size_t)1 << 40), cap, nullptr), "too large"), "elems too large");
  expect(refused(vcg_pool_exchange(fake, pool, out, ok, N, SIZE_MAX, INT_MAX, nullptr), "too large"), "elems = SIZE_MAX");
  const int32_t bad_entries[] = {cap, cap + 1, -(2 + cap), -(3 + cap), INT32_MAX, INT32_MIN};
  for (int32_t e : bad_entries) {
    const int32_t first[2] = {e, 0}, second[2] = {-1, e};
    expect(refused(vcg_pool_exchange(fake, pool, out, first, N, elems, cap, nullptr), "plan[0]"), "a first entry outside the three forms");
    expect(refused(vcg_pool_exchange(fake, pool, out, second, N, elems, cap, nullptr), "plan[1]"), "a second entry outside the three forms");
  }
  expect(refused(vcg_pool_exchange(fake, pool, fake, ok, N, elems, cap, nullptr), "overlap"), "out is fake");
  expect(refused(vcg_pool_exchange(fake, pool, fake + 28, ok, N, elems, cap, nullptr), "overlap"), "out begins in fake's last words");
  expect(refused(vcg_pool_exchange(fake + 28, pool, fake, ok, N, elems, cap, nullptr), "overlap"), "fake begins in out's last words");
  expect(refused(vcg_pool_exchange(fake, fake + 16, buf + 128, ok, N, elems, cap, nullptr), "overlap"), "pool begins inside fake");
  expect(refused(vcg_pool_exchange(buf + 124, pool, buf + 160, ok, N, elems, cap, nullptr), "overlap"), "fake begins in the pool's last slot");
  expect(refused(vcg_pool_exchange(fake, pool, buf + 96, ok, N, elems, cap, nullptr), "overlap"), "out inside the pool");
  expect(refused(vcg_pool_exchange(fake, pool, buf + 36, ok, N, elems, cap, nullptr), "overlap"), "out ends inside the pool");
  expect(vcg_pool_exchange(fake, pool, out, ok, 0, elems, cap, nullptr) == 0, "N == 0 is a no-op");
  expect(vcg_pool_exchange(fake, pool, out, ok, 0, 0, cap, nullptr) == 0, "N == 0, elems == 0 is a no-op");

  for (int i = 0; i < 256; ++i) expect(buf[i] == (float)i, "a refused or empty call wrote to its arguments");
  free(buf);
  if (failures) return 1;
  puts("image_pool_host_check: ok");
  return 0;
}
