// The sampling translator (translate.py --samples K): K decodes of one encoder pass, their running mean and spread.
// New: the reference has no inference path.
//
//   vcg_reparam_many_fwd   z[(n, j)] = mu[n] + temperature * eps[(n, j)] * exp(0.5 * clamp(lv[n], -10, 10)) for a chunk of the K
//                          samples of each of N latent maps.  Sample (n, j) draws the quads vcg_randn(seed, offset + (n K + j) per / 4)
//                          would write: a function of (seed, offset, n, j), not of the chunking.
//   vcg_sample_accumulate  Welford's running mean and sum of squared deviations of clamp(y, 0, 1) over the samples, one float4 per
//                          lane, the chunk's samples folded in order.  ONE loop body serves every chunking and the file is compiled
//                          with contraction off (the one fused operation is written as fmaf): an element's operation sequence, and
//                          so its bits, do not depend on how the K samples were split into calls.
//   vcg_spread_display_hw  per pixel of a window the RMS over the three channels of the unbiased sample standard deviation, as
//                          fp32 and / or a grey uint8 map, and its mean per image: metrics.hip's scheme (each 16 x 16 tile a slot of
//                          its own, in double; a final pass sums an image's slots in a fixed order; no float atomics).
//
// All three stream their operands once with 16-byte loads and stores; none has a reduction across lanes except the spread's mean.
#include <math.h>

#include "vcg_common.h"

#pragma clang fp contract(off)

#define SS_THREADS 256
#define SS_MAX_BLOCKS 2048
#define SS_TILE 16

static int ss_blocks(size_t work) {
  size_t b = (work + SS_THREADS - 1) / SS_THREADS;
  if (b > SS_MAX_BLOCKS) b = SS_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

static inline bool ss_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------- reparameterisation of a chunk of samples
// quad q of the chunk's (N, k, per / 4) output; mu / lv quad (n, i); drawn eps: counter offset + ((n K + first + j) per4 + i).
// z = fmaf(temperature * eps, sd, mu): for temperature == 1 k_reparam_fwd's mu + eps * sd as hipcc contracts it (misc.hip is
// compiled with contraction on); temperature == 0 returns mu's own bits (a sum would turn -0 into +0).
__global__ __launch_bounds__(SS_THREADS) void k_reparam_many(const float4* __restrict__ mu, const float4* __restrict__ lv,
                                                             const float4* __restrict__ eps, float4* __restrict__ eps_out,
                                                             float4* __restrict__ z, size_t total, size_t per4, int K, int first, int k,
                                                             float temperature, uint64_t seed, uint64_t offset) {
  const size_t chunk4 = (size_t)k * per4;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const size_t n = q / chunk4, r = q - n * chunk4, j = r / per4, i = r - j * per4;
    const float4 m = mu[n * per4 + i], l = lv[n * per4 + i];
    const float4 e = eps ? eps[q] : randn4(seed, offset + ((n * (size_t)K + (size_t)first + j) * per4 + i));
    const float mv[4] = {m.x, m.y, m.z, m.w}, lvv[4] = {l.x, l.y, l.z, l.w}, ev[4] = {e.x, e.y, e.z, e.w};
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float sd = expf(0.5f * fminf(fmaxf(lvv[c], -10.f), 10.f));
      o[c] = temperature == 0.f ? mv[c] : fmaf(temperature * ev[c], sd, mv[c]);
    }
    z[q] = make_float4(o[0], o[1], o[2], o[3]);
    if (eps_out) eps_out[q] = e;
  }
}

extern "C" int vcg_reparam_many_fwd(const float* mu, const float* lv, const float* eps, float* eps_out, float* z, int N, int K,
                                    int first, int k, size_t per, float temperature, uint64_t seed, uint64_t offset, void* stream) {
  VCG_CHECK_ARG(mu && lv && z, "vcg_reparam_many_fwd: null pointer");
  VCG_CHECK_ARG(N >= 1 && K >= 1 && k >= 1, "vcg_reparam_many_fwd: N=%d, K=%d, k=%d must all be at least 1", N, K, k);
  VCG_CHECK_ARG(first >= 0 && (long long)first + k <= K, "vcg_reparam_many_fwd: samples %d .. %lld leave the %d of the batch", first,
                (long long)first + k - 1, K);
  VCG_CHECK_ARG(per >= 4 && per % 4 == 0 && per <= ((size_t)1 << 31), "vcg_reparam_many_fwd: per=%zu must be a positive multiple of 4", per);
  VCG_CHECK_ARG(isfinite(temperature) && temperature >= 0.f, "vcg_reparam_many_fwd: temperature must be finite and >= 0, got %g",
                (double)temperature);
  VCG_CHECK_ARG(ss_aligned16(mu) && ss_aligned16(lv) && ss_aligned16(z) && ss_aligned16(eps) && ss_aligned16(eps_out),
                "vcg_reparam_many_fwd: a pointer is not 16-byte aligned");
  const size_t per4 = per / 4, total = (size_t)N * k * per4;
  hipLaunchKernelGGL(k_reparam_many, dim3(ss_blocks(total)), dim3(SS_THREADS), 0, (hipStream_t)stream, (const float4*)mu,
                     (const float4*)lv, (const float4*)eps, (float4*)eps_out, (float4*)z, total, per4, K, first, k, temperature, seed,
                     offset);
  VCG_LAUNCH_CHECK("vcg_reparam_many_fwd");
  return 0;
}

// ---------------------------------------------------------------- running mean and spread over the samples
__device__ __forceinline__ float ss_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// one Welford update of one value: d / c is an IEEE division, the product enters m2 through one fmaf
__device__ __forceinline__ void ss_fold(float x, float c, float& mean, float& m2) {
  const float d = x - mean;
  mean = mean + d / c;
  m2 = fmaf(d, x - mean, m2);
}

// element e = (n, pixel): y[(n k + j) pixels + pixel] for j = 0 .. k-1; seen == 0 starts from zeros without reading mean / m2
__global__ __launch_bounds__(SS_THREADS) void k_sample_accumulate(const float4* __restrict__ y, float4* __restrict__ mean,
                                                                  float4* __restrict__ m2, size_t total, size_t pixels, int k, int seen) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t n = e / pixels, p = e - n * pixels;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), s = a;
    if (seen > 0) {
      a = mean[e];
      s = m2[e];
    }
    const float4* src = y + (n * (size_t)k) * pixels + p;
    for (int j = 0; j < k; ++j) {
      const float4 v = src[(size_t)j * pixels];
      const float c = (float)(seen + j + 1);
      ss_fold(ss_clamp01(v.x), c, a.x, s.x);
      ss_fold(ss_clamp01(v.y), c, a.y, s.y);
      ss_fold(ss_clamp01(v.z), c, a.z, s.z);
    }
    a.w = 0.f;
    s.w = 0.f;
    mean[e] = a;
    m2[e] = s;
  }
}

extern "C" int vcg_sample_accumulate(const float* y, float* mean, float* m2, int N, int k, int seen, size_t pixels, void* stream) {
  VCG_CHECK_ARG(y && mean && m2, "vcg_sample_accumulate: null pointer");
  VCG_CHECK_ARG(N >= 1 && k >= 1, "vcg_sample_accumulate: N=%d and k=%d must be at least 1", N, k);
  VCG_CHECK_ARG(seen >= 0 && (long long)seen + k <= (1 << 24), "vcg_sample_accumulate: seen=%d, k=%d: the count must stay exact in fp32",
                seen, k);
  VCG_CHECK_ARG(pixels >= 1 && pixels <= ((size_t)1 << 31), "vcg_sample_accumulate: pixels=%zu", pixels);
  VCG_CHECK_ARG(ss_aligned16(y) && ss_aligned16(mean) && ss_aligned16(m2), "vcg_sample_accumulate: a pointer is not 16-byte aligned");
  VCG_CHECK_ARG(mean != m2, "vcg_sample_accumulate: mean and m2 are one buffer");
  const size_t total = (size_t)N * pixels;
  hipLaunchKernelGGL(k_sample_accumulate, dim3(ss_blocks(total)), dim3(SS_THREADS), 0, (hipStream_t)stream, (const float4*)y,
                     (float4*)mean, (float4*)m2, total, pixels, k, seen);
  VCG_LAUNCH_CHECK("vcg_sample_accumulate");
  return 0;
}

// ---------------------------------------------------------------- the spread map
struct SpreadP {
  const float4* m2;       // (N, Hp, Wp, 4): sums of squared deviations of `count` samples; the window (top, left, H, W) is read
  float* out_f32;         // (N, H, W) or null
  unsigned char* out_u8;  // (N, H, W) or null
  double* ws;             // [N][tiles]: each tile's sum of s
  float* res;             // [N]
  int H, W, Hp, Wp, top, left, tiles_x, tiles_y;
  double den;             // 3 (count - 1)
  double gain;
};

// one workgroup per 16 x 16 tile of the window.  s is evaluated in double and rounded once: the fp32 map is the correctly rounded
// value up to the double's own error, and the uint8 map is the floor of the unrounded 255 min(1, gain s) + 0.5 (k_to_display's rule).
__global__ __launch_bounds__(SS_TILE * SS_TILE) void k_spread(SpreadP p) {
  __shared__ double red[SS_TILE * SS_TILE];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int y = blockIdx.y * SS_TILE + tid / SS_TILE, x = blockIdx.x * SS_TILE + tid % SS_TILE;
  double s = 0.0;
  if (y < p.H && x < p.W) {                  // nothing outside the window is read
    const float4 v = p.m2[((size_t)n * p.Hp + p.top + y) * p.Wp + p.left + x];
    s = sqrt(((double)v.x + (double)v.y + (double)v.z) / p.den);
    const size_t i = ((size_t)n * p.H + y) * p.W + x;
    if (p.out_f32) p.out_f32[i] = (float)s;
    if (p.out_u8) p.out_u8[i] = (unsigned char)floor(255.0 * fmin(1.0, p.gain * s) + 0.5);
  }
  red[tid] = s;
  __syncthreads();
  for (int h = SS_TILE * SS_TILE / 2; h > 0; h >>= 1) {   // fixed-order tree
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) p.ws[((size_t)n * p.tiles_y + blockIdx.y) * p.tiles_x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_spread_final(SpreadP p) {
  __shared__ double red[256];
  const int n = blockIdx.x, tid = threadIdx.x, tiles = p.tiles_x * p.tiles_y;
  const double* ws = p.ws + (size_t)n * tiles;
  double a = 0.0;
  for (int i = tid; i < tiles; i += 256) a += ws[i];      // each thread a fixed strided subset, in order
  red[tid] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) p.res[n] = (float)(red[0] / ((double)p.H * (double)p.W));
}

extern "C" size_t vcg_spread_workspace(int N, int H, int W) {
  if (N < 1 || N > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535) {
    vcg_set_error("vcg_spread_workspace: bad N=%d H=%d W=%d", N, H, W);
    return 0;
  }
  const size_t tiles = (size_t)((H + SS_TILE - 1) / SS_TILE) * ((W + SS_TILE - 1) / SS_TILE);
  return ((size_t)N * tiles * sizeof(double) + 15) / 16 * 16;
}

extern "C" int vcg_spread_display_hw(const float* m2, int count, float gain, float* out_f32, unsigned char* out_u8, float* result, int N,
                                     int Hp, int Wp, int top, int left, int H, int W, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(m2 && result && ws, "vcg_spread_display_hw: null pointer");
  VCG_CHECK_ARG(count >= 2, "vcg_spread_display_hw: a spread needs at least 2 samples, got count=%d", count);
  VCG_CHECK_ARG(isfinite(gain) && gain >= 0.f, "vcg_spread_display_hw: gain must be finite and >= 0, got %g", (double)gain);
  VCG_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && Hp <= 65535 && Wp <= 65535, "vcg_spread_display_hw: bad N=%d H=%d W=%d", N,
                H, W);
  VCG_CHECK_ARG(top >= 0 && left >= 0 && (long long)top + H <= Hp && (long long)left + W <= Wp,
                "vcg_spread_display_hw: the %dx%d window at (%d, %d) leaves the %dx%d buffer", H, W, top, left, Hp, Wp);
  VCG_CHECK_ARG(ss_aligned16(m2) && ss_aligned16(ws) && ((uintptr_t)out_f32 & 3) == 0 && ((uintptr_t)result & 3) == 0,
                "vcg_spread_display_hw: m2 and ws must be 16-byte aligned, out_f32 and result 4-byte aligned");
  const size_t need = vcg_spread_workspace(N, H, W);
  VCG_CHECK_ARG(ws_bytes >= need, "vcg_spread_display_hw: workspace of %zu bytes, %zu needed", ws_bytes, need);
  SpreadP p;
  p.m2 = (const float4*)m2; p.out_f32 = out_f32; p.out_u8 = out_u8; p.ws = (double*)ws; p.res = result;
  p.H = H; p.W = W; p.Hp = Hp; p.Wp = Wp; p.top = top; p.left = left;
  p.tiles_x = (W + SS_TILE - 1) / SS_TILE;
  p.tiles_y = (H + SS_TILE - 1) / SS_TILE;
  p.den = 3.0 * (double)(count - 1);
  p.gain = (double)gain;
  hipLaunchKernelGGL(k_spread, dim3(p.tiles_x, p.tiles_y, N), dim3(SS_TILE * SS_TILE), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(k_spread_final, dim3(N), dim3(256), 0, (hipStream_t)stream, p);
  VCG_LAUNCH_CHECK("vcg_spread_display_hw");
  return 0;
}
