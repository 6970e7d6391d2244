// Exponential moving average of the optimizer's flat parameter buffer, and the in-place exchange of two flat buffers that puts
// the average in the parameters' place for an evaluation and takes it out again.  Kernels of their own: k_adam (misc.hip) is not
// touched, and a run without an average launches neither.
//
//   vcg_ema_update:  e[i] = fmaf(w, p[i] - e[i], e[i]),  w = (float)(1 - decay), rounded once from double by the caller.
//                    12 B per parameter (read p, read e, write e) beside the Adam launch's 28.
//   vcg_swap:        a[i] <-> b[i], 16 B per element, one pass, no workspace.
//
// Both are k_adam's shape: one float4 per lane, grid-stride, at most EMA_MAX_BLOCKS workgroups of EMA_THREADS lanes (8 per CU:
// 32 waves per CU with two 16-byte loads each in flight), and the n % 4 last elements by workgroup 0.  Every access is a vector
// load or store; nothing is accumulated across lanes, so a call is a pure function of its inputs.
#include <math.h>

#include "vcg_common.h"

#define EMA_THREADS 256
#define EMA_MAX_BLOCKS 2048

static int ema_blocks(size_t n4) {
  size_t b = (n4 + EMA_THREADS - 1) / EMA_THREADS;
  if (b > EMA_MAX_BLOCKS) b = EMA_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

// COPY (w == 1.0f): e = p exactly — fmaf(1, p - e, e) is not p in general (p - e is rounded).
// skip: the four floats vcg_grad_norm left (grad_clip.hip), or null.  skip[2] != 0: the Adam launch before this one wrote nothing,
// and neither does this one.
template <bool COPY>
__global__ __launch_bounds__(EMA_THREADS) void k_ema(float* __restrict__ e, const float* __restrict__ p, size_t n, float w,
                                                     const float* __restrict__ skip) {
  if (skip && skip[2] != 0.f) return;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 pv = reinterpret_cast<const float4*>(p)[i];
    if (COPY) {
      reinterpret_cast<float4*>(e)[i] = pv;
    } else {
      float4 ev = reinterpret_cast<float4*>(e)[i];
      ev.x = fmaf(w, pv.x - ev.x, ev.x);
      ev.y = fmaf(w, pv.y - ev.y, ev.y);
      ev.z = fmaf(w, pv.z - ev.z, ev.z);
      ev.w = fmaf(w, pv.w - ev.w, ev.w);
      reinterpret_cast<float4*>(e)[i] = ev;
    }
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) e[i] = COPY ? p[i] : fmaf(w, p[i] - e[i], e[i]);
}

// words, not floats: a NaN keeps its payload
__global__ __launch_bounds__(EMA_THREADS) void k_swap(uint32_t* __restrict__ a, uint32_t* __restrict__ b, size_t n) {
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const uint4 av = reinterpret_cast<uint4*>(a)[i];
    const uint4 bv = reinterpret_cast<uint4*>(b)[i];
    reinterpret_cast<uint4*>(a)[i] = bv;
    reinterpret_cast<uint4*>(b)[i] = av;
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      const uint32_t av = a[i];
      a[i] = b[i];
      b[i] = av;
    }
}

extern "C" int vcg_ema_update(float* e, const float* p, size_t n, float w, const float* skip, void* stream) {
  VCG_CHECK_ARG(e && p, "vcg_ema_update: null pointer");
  VCG_CHECK_ARG(isfinite(w) && w >= 0.f && w <= 1.f, "vcg_ema_update: w = 1 - decay must lie in [0, 1], got %g", (double)w);
  VCG_CHECK_ARG((((uintptr_t)e | (uintptr_t)p) & 15) == 0, "vcg_ema_update: e or p not 16-byte aligned");
  VCG_CHECK_ARG(n <= ((size_t)1 << 40), "vcg_ema_update: n=%zu is too large", n);
  if (n == 0 || w == 0.f) return 0;                     // w == 0: e keeps its bits (a launch would turn e + 0 * inf into NaN)
  const dim3 grid(ema_blocks(n / 4)), block(EMA_THREADS);
  if (w == 1.f)
    hipLaunchKernelGGL(k_ema<true>, grid, block, 0, (hipStream_t)stream, e, p, n, w, skip);
  else
    hipLaunchKernelGGL(k_ema<false>, grid, block, 0, (hipStream_t)stream, e, p, n, w, skip);
  VCG_LAUNCH_CHECK("vcg_ema_update");
  return 0;
}

extern "C" int vcg_swap(float* a, float* b, size_t n, void* stream) {
  VCG_CHECK_ARG(a && b, "vcg_swap: null pointer");
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "vcg_swap: a or b not 16-byte aligned");
  VCG_CHECK_ARG(n <= ((size_t)1 << 40), "vcg_swap: n=%zu is too large", n);
  if (n == 0) return 0;
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  VCG_CHECK_ARG(ua + bytes <= ub || ub + bytes <= ua, "vcg_swap: the two ranges overlap");
  hipLaunchKernelGGL(k_swap, dim3(ema_blocks(n / 4)), dim3(EMA_THREADS), 0, (hipStream_t)stream, (uint32_t*)a, (uint32_t*)b, n);
  VCG_LAUNCH_CHECK("vcg_swap");
  return 0;
}
