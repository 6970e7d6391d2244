// Global 2-norm of the optimizer's flat gradient buffer and the clip coefficient torch.nn.utils.clip_grad_norm_ would apply,
// left on the device for the Adam launch that follows (k_adam<true>, misc.hip): no host round-trip, no pass that rescales the
// gradients in place.
//
//   out[0] = |grad_scale| sqrt(sum g[i]^2)                   the norm of the gradient Adam sees (grad_scale = 1 / world after a
//                                                            summing all-reduce), rounded once to fp32; +inf if it exceeds fp32
//   out[1] = min(1, max_norm / (norm + 1e-6))                torch's formula and constant, in double from the unrounded norm
//   out[2] = 1 if any g[i] is NaN or +-Inf, else 0           decided from the double sum, never from out[0]
//   out[3] = 0
//
// Every element is squared and summed in double: the square of an fp32 value is exact there (24 x 24 bits) and the sum of up to
// 2^40 squares of 3.4e38 stays below 1e90, so a non-finite sum means a non-finite element and nothing else.
// k_grad_norm_partial: one workgroup per fixed chunk of GN_CHUNK4 float4 (64 KiB of g, 16 float4 per lane, issued before the
// first is used), lanes sum their elements in index order, wave butterfly, four wave sums through LDS, one slot per workgroup.
// k_grad_norm_final (one workgroup): each lane sums a fixed strided subset of the slots in order, the n % 4 tail elements join
// lanes 0..2, fixed tree, lane 0 writes `out` as one float4.  The grid depends on n alone and no float atomic is used: the same
// input gives the same bits on every call (the scheme of ssim_loss.hip and metrics.hip).
#include <math.h>

#include "vcg_common.h"

#define GN_THREADS 256
#define GN_PER_LANE 16
#define GN_CHUNK4 (GN_THREADS * GN_PER_LANE)   // float4 per workgroup; GN_CHUNK = 16384 floats (vcg.h states the formula)

__device__ __forceinline__ double gn_sq4(double s, const float4 v) {
  const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
  s += x * x; s += y * y; s += z * z; s += w * w;
  return s;
}

__global__ __launch_bounds__(GN_THREADS) void k_grad_norm_partial(const float4* __restrict__ g, size_t n4, double* __restrict__ slots) {
  __shared__ double red[GN_THREADS / VCG_WAVE];
  const int tid = threadIdx.x;
  const size_t lo = (size_t)blockIdx.x * GN_CHUNK4;
  const size_t hi = lo + GN_CHUNK4 < n4 ? lo + GN_CHUNK4 : n4;
  double s = 0.0;
  if (hi - lo == GN_CHUNK4) {
    float4 v[GN_PER_LANE];
#pragma unroll
    for (int k = 0; k < GN_PER_LANE; ++k) v[k] = g[lo + (size_t)k * GN_THREADS + tid];
#pragma unroll
    for (int k = 0; k < GN_PER_LANE; ++k) s = gn_sq4(s, v[k]);
  } else {
    for (size_t i = lo + tid; i < hi; i += GN_THREADS) s = gn_sq4(s, g[i]);        // the last chunk: same elements per lane, same order
  }
  s = wave_sum_d(s);
  if ((tid & (VCG_WAVE - 1)) == 0) red[tid / VCG_WAVE] = s;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
#pragma unroll
    for (int w = 1; w < GN_THREADS / VCG_WAVE; ++w) t += red[w];
    slots[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(GN_THREADS) void k_grad_norm_final(const double* __restrict__ slots, int nslots, const float* __restrict__ g,
                                                                size_t n, float gscale, float max_norm, float4* __restrict__ out) {
  __shared__ double red[GN_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < nslots; i += GN_THREADS) s += slots[i];       // each lane a fixed strided subset, in order
  const size_t t0 = n & ~(size_t)3;                                   // the n % 4 elements no float4 covers
  if (t0 + tid < n) {
    const double x = (double)g[t0 + tid];
    s += x * x;
  }
  red[tid] = s;
  __syncthreads();
  for (int h = GN_THREADS / 2; h > 0; h >>= 1) {                       // fixed-order tree
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double total = red[0];
    const double norm = fabs((double)gscale) * sqrt(total);
    const double coef = fmin(1.0, (double)max_norm / (norm + 1e-6));  // a NaN norm gives 1: the step is skipped anyway
    out[0] = make_float4((float)norm, (float)coef, isfinite(total) ? 0.f : 1.f, 0.f);
  }
}

static size_t gn_slots(size_t n) { return (n / 4 + GN_CHUNK4 - 1) / GN_CHUNK4; }

extern "C" size_t vcg_grad_norm_workspace(size_t n) {
  const size_t slots = gn_slots(n);
  return ((slots > 0 ? slots : 1) * sizeof(double) + 15) / 16 * 16;
}

extern "C" int vcg_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, float* out, void* ws, size_t ws_bytes,
                             void* stream) {
  VCG_CHECK_ARG(g && out && ws, "vcg_grad_norm: null pointer");
  VCG_CHECK_ARG(isfinite(max_norm) && max_norm > 0.f, "vcg_grad_norm: max_norm must be finite and > 0, got %g", (double)max_norm);
  VCG_CHECK_ARG(isfinite(grad_scale), "vcg_grad_norm: grad_scale must be finite, got %g", (double)grad_scale);
  const size_t slots = gn_slots(n);
  VCG_CHECK_ARG(slots <= 0x7FFFFFFFu, "vcg_grad_norm: n=%zu is too large", n);
  const size_t need = vcg_grad_norm_workspace(n);
  VCG_CHECK_ARG(ws_bytes >= need, "vcg_grad_norm: workspace of %zu bytes, %zu needed", ws_bytes, need);
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_grad_norm: workspace not 16-byte aligned");
  VCG_CHECK_ARG((((uintptr_t)g | (uintptr_t)out) & 15) == 0, "vcg_grad_norm: g or out not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (slots > 0)
    hipLaunchKernelGGL(k_grad_norm_partial, dim3((unsigned)slots), dim3(GN_THREADS), 0, st, (const float4*)g, n / 4, (double*)ws);
  hipLaunchKernelGGL(k_grad_norm_final, dim3(1), dim3(GN_THREADS), 0, st, (const double*)ws, (int)slots, g, n, grad_scale, max_norm,
                     (float4*)out);
  VCG_LAUNCH_CHECK("vcg_grad_norm");
  return 0;
}
