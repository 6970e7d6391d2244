// The adversarial terms of one discriminator's (real, fake) logit pair under a selectable objective (new: the reference has LSGAN
// alone).  Kernels of their own: the LSGAN path of the default configuration (k_mse_const_fwd / k_mse_const_bwd in misc.hip) is
// not touched, and a run with the default objective launches none of these.
//
//   real, fake: dense fp32 logits, n_real and n_fake of them (batch x head positions: a few thousand at most).  Either side may
//   be absent (null, count 0) — the image-pool path has the fake side alone — but not both.  With s the label smoothing and
//   sp(t) = max(t, 0) + log1p(exp(-|t|)), every term is the mean over its tensor of
//
//     objective   D real                      D fake         G real   G fake
//     lsgan       (z - (1 - s))^2             z^2            z^2      (z - 1)^2
//     hinge       max(0, 1 - z)               max(0, 1 + z)  z        -z
//     logistic    (1 - s) sp(-z) + s sp(z)    sp(z)          sp(z)    sp(-z)
//
//   forward, one launch of two workgroups of 256 threads: workgroup 0 reduces `real`, workgroup 1 `fake`.  A thread strides over
//   its side, evaluates every summand in double from the exactly converted logit and sums in double; the 64 lanes of a wavefront
//   are combined by a butterfly of shuffles, the four wavefronts through LDS in wavefront order, and thread 0 divides by the count
//   and rounds ONCE to fp32:  out = [g_real, g_fake, d_real, d_fake, mean_real, mean_fake], the slots of an absent side 0.
//   backward, one elementwise launch over both sides:  g_z[i] = (gG G'(z) + gD D'(z)) / n, in double, rounded once.
//
// No atomics, every sum in a fixed order: the same input gives the same bits.  A NaN logit reaches its side's terms (the hinge is
// written as a select that a NaN falls through, not as fmax); an infinite logit gives the limit, never a NaN of the arithmetic
// (a smoothing of 0 skips its term instead of multiplying it by 0).  The hinge's derivative at its kink is 0, as torch.relu's.
#include <math.h>

#include "vcg_common.h"

#define GANT_THREADS 256
#define GANT_WAVES (GANT_THREADS / 64)
#define GANT_BWD_MAX_BLOCKS 1024

enum { GANT_LSGAN = VCG_GAN_LSGAN, GANT_HINGE = VCG_GAN_HINGE, GANT_LOGISTIC = VCG_GAN_LOGISTIC };

__device__ __forceinline__ double gant_softplus(double t) { return (t > 0.0 ? t : 0.0) + log1p(exp(-fabs(t))); }
// d/dt softplus: the logistic function, without an overflowing exp
__device__ __forceinline__ double gant_sigmoid(double t) {
  const double e = exp(-fabs(t));
  return (t >= 0.0 ? 1.0 : e) / (1.0 + e);
}
// max(0, t) that a NaN falls through
__device__ __forceinline__ double gant_relu(double t) { return t < 0.0 ? 0.0 : t; }
// d/dt max(0, t): 0 at the kink; a NaN stays one
__device__ __forceinline__ double gant_step(double t) { return t > 0.0 ? 1.0 : (t != t ? t : 0.0); }

// (generator summand, discriminator summand) of logit z on side `fake`
template <int OBJ>
__device__ __forceinline__ void gant_terms(double z, bool fake, double s, double& g, double& d) {
  if (OBJ == GANT_LSGAN) {
    const double a = fake ? z - 1.0 : z, b = fake ? z : z - (1.0 - s);
    g = a * a;
    d = b * b;
  } else if (OBJ == GANT_HINGE) {
    g = fake ? -z : z;
    d = gant_relu(fake ? 1.0 + z : 1.0 - z);
  } else {
    const double up = gant_softplus(z), down = gant_softplus(-z);
    g = fake ? down : up;
    if (fake) {
      d = up;
    } else {
      d = (1.0 - s) * down;
      if (s != 0.0) d += s * up;                  // s = 0 at z = +inf: no 0 x inf
    }
  }
}

// their derivatives in z
template <int OBJ>
__device__ __forceinline__ void gant_slopes(double z, bool fake, double s, double& g, double& d) {
  if (OBJ == GANT_LSGAN) {
    g = 2.0 * (fake ? z - 1.0 : z);
    d = 2.0 * (fake ? z : z - (1.0 - s));
  } else if (OBJ == GANT_HINGE) {
    g = fake ? -1.0 : 1.0;
    d = fake ? gant_step(1.0 + z) : -gant_step(1.0 - z);
  } else {
    const double up = gant_sigmoid(z), down = gant_sigmoid(-z);
    g = fake ? -down : up;
    if (fake) {
      d = up;
    } else {
      d = -(1.0 - s) * down;
      if (s != 0.0) d += s * up;
    }
  }
}

// grid 2: blockIdx.x = 0 the real side, 1 the fake side
template <int OBJ>
__global__ __launch_bounds__(GANT_THREADS) void k_gan_terms_fwd(const float* __restrict__ real, size_t n_real,
                                                                const float* __restrict__ fake, size_t n_fake, double s,
                                                                float* __restrict__ out) {
  __shared__ double red[3][GANT_WAVES];
  const bool side = blockIdx.x != 0;
  const float* __restrict__ z = side ? fake : real;
  const size_t n = side ? n_fake : n_real;
  double sg = 0.0, sd = 0.0, sm = 0.0;
  for (size_t i = threadIdx.x; i < n; i += GANT_THREADS) {
    const double v = (double)z[i];
    double g, d;
    gant_terms<OBJ>(v, side, s, g, d);
    sg += g;
    sd += d;
    sm += v;
  }
  sg = wave_sum_d(sg);
  sd = wave_sum_d(sd);
  sm = wave_sum_d(sm);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = sg;
    red[1][wave] = sd;
    red[2][wave] = sm;
  }
  __syncthreads();
  if (threadIdx.x < 3) {                           // lane k of the first wavefront finishes sum k: wavefront order, one rounding
    double v = red[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < GANT_WAVES; ++w) v += red[threadIdx.x][w];
    out[2 * threadIdx.x + (side ? 1 : 0)] = n ? (float)(v / (double)n) : 0.f;
  }
}

struct GantUpstream {
  const float* g[4];                              // d loss / d [g_real, g_fake, d_real, d_fake]; null: that term is not differentiated
};

// one thread per logit of either side: i < n_real the real side, the rest the fake side
template <int OBJ>
__global__ __launch_bounds__(GANT_THREADS) void k_gan_terms_bwd(const float* __restrict__ real, size_t n_real,
                                                                const float* __restrict__ fake, size_t n_fake, double s,
                                                                GantUpstream up, float* __restrict__ g_real,
                                                                float* __restrict__ g_fake) {
  const size_t n = n_real + n_fake;
  for (size_t i = (size_t)blockIdx.x * GANT_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * GANT_THREADS) {
    const bool side = i >= n_real;
    const size_t j = side ? i - n_real : i;
    const float* pg = up.g[side ? 1 : 0];
    const float* pd = up.g[side ? 3 : 2];
    double sg, sd, acc = 0.0;
    gant_slopes<OBJ>((double)(side ? fake : real)[j], side, s, sg, sd);
    if (pg) acc += (double)pg[0] * sg;
    if (pd) acc += (double)pd[0] * sd;
    (side ? g_fake : g_real)[j] = (float)(acc / (double)(side ? n_fake : n_real));
  }
}

static int gant_check(const char* who, const float* real, size_t n_real, const float* fake, size_t n_fake, int objective,
                      double smooth) {
  VCG_CHECK_ARG(objective == GANT_LSGAN || objective == GANT_HINGE || objective == GANT_LOGISTIC,
                "%s: unknown objective %d (0 lsgan, 1 hinge, 2 logistic)", who, objective);
  VCG_CHECK_ARG(isfinite(smooth) && smooth >= 0.0 && smooth < 0.5, "%s: the label smoothing must lie in [0, 0.5), got %g", who,
                smooth);
  VCG_CHECK_ARG(objective != GANT_HINGE || smooth == 0.0, "%s: the hinge objective takes no label smoothing, got %g", who, smooth);
  VCG_CHECK_ARG((real != nullptr) == (n_real != 0) && (fake != nullptr) == (n_fake != 0),
                "%s: a side is present with a pointer and a count, or absent with neither (real %p x %zu, fake %p x %zu)", who,
                (const void*)real, n_real, (const void*)fake, n_fake);
  VCG_CHECK_ARG(n_real + n_fake > 0, "%s: both sides are absent", who);
  VCG_CHECK_ARG(n_real <= ((size_t)1 << 40) && n_fake <= ((size_t)1 << 40), "%s: a side has more than 2^40 logits", who);
  return 0;
}

extern "C" int vcg_gan_terms_fwd(const float* real, size_t n_real, const float* fake, size_t n_fake, int objective, double smooth,
                                 float* out, void* stream) {
  if (gant_check("vcg_gan_terms_fwd", real, n_real, fake, n_fake, objective, smooth)) return -1;
  VCG_CHECK_ARG(out, "vcg_gan_terms_fwd: null output");
  hipStream_t st = (hipStream_t)stream;
  if (objective == GANT_LSGAN)
    hipLaunchKernelGGL(k_gan_terms_fwd<GANT_LSGAN>, dim3(2), dim3(GANT_THREADS), 0, st, real, n_real, fake, n_fake, smooth, out);
  else if (objective == GANT_HINGE)
    hipLaunchKernelGGL(k_gan_terms_fwd<GANT_HINGE>, dim3(2), dim3(GANT_THREADS), 0, st, real, n_real, fake, n_fake, smooth, out);
  else
    hipLaunchKernelGGL(k_gan_terms_fwd<GANT_LOGISTIC>, dim3(2), dim3(GANT_THREADS), 0, st, real, n_real, fake, n_fake, smooth, out);
  VCG_LAUNCH_CHECK("vcg_gan_terms_fwd");
  return 0;
}

extern "C" int vcg_gan_terms_bwd(const float* real, size_t n_real, const float* fake, size_t n_fake, int objective, double smooth,
                                 const float* const* g_out, float* g_real, float* g_fake, void* stream) {
  if (gant_check("vcg_gan_terms_bwd", real, n_real, fake, n_fake, objective, smooth)) return -1;
  VCG_CHECK_ARG(g_out, "vcg_gan_terms_bwd: null upstream table");
  VCG_CHECK_ARG((g_real || !n_real) && (g_fake || !n_fake), "vcg_gan_terms_bwd: a present side has no gradient buffer");
  GantUpstream up;
  for (int k = 0; k < 4; ++k) up.g[k] = g_out[k];
  const size_t n = n_real + n_fake;
  size_t blocks = (n + GANT_THREADS - 1) / GANT_THREADS;
  if (blocks > GANT_BWD_MAX_BLOCKS) blocks = GANT_BWD_MAX_BLOCKS;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(GANT_THREADS);
  if (objective == GANT_LSGAN)
    hipLaunchKernelGGL(k_gan_terms_bwd<GANT_LSGAN>, grid, block, 0, st, real, n_real, fake, n_fake, smooth, up, g_real, g_fake);
  else if (objective == GANT_HINGE)
    hipLaunchKernelGGL(k_gan_terms_bwd<GANT_HINGE>, grid, block, 0, st, real, n_real, fake, n_fake, smooth, up, g_real, g_fake);
  else
    hipLaunchKernelGGL(k_gan_terms_bwd<GANT_LOGISTIC>, grid, block, 0, st, real, n_real, fake, n_fake, smooth, up, g_real, g_fake);
  VCG_LAUNCH_CHECK("vcg_gan_terms_bwd");
  return 0;
}
