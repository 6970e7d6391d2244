// The 11 x 11 Gaussian window of the structural losses (ssim_loss.hip, msssim_loss.hip): tile geometry, the staging and the two
// separable passes with the five moments summed in double about a per-tile shift, and the per-position values and derivative
// coefficients.  The helpers are templates on the kernel's parameter struct P, which holds a, b (const float4*, (N, H, W, 4)),
// H, W and the window w[SL_WIN]; ssim_loss.hip's header comment has the formulas.
#pragma once
#include <math.h>

#include "vcg_common.h"

#define SL_WIN 11
#define SL_HALO (SL_WIN - 1)
#define SL_TILE 16
#define SL_THREADS (SL_TILE * SL_TILE)
#define SL_FP SL_TILE                     // forward: positions per tile side
#define SL_FS (SL_FP + SL_HALO)           // 26: pixels staged per side
#define SL_BP (SL_TILE + SL_HALO)         // backward: 26 positions per side reach the tile's pixels
#define SL_BS (SL_BP + SL_HALO)           // 36: pixels staged per side

// pixels (sy + r, sx + c), r, c < S, of image n, minus the shift; outside the image 0 (read by positions that are not valid only)
template <int S, class P>
__device__ __forceinline__ void sl_stage(const P& p, int n, int sy, int sx, const float* ka, const float* kb, float (*sa)[S * S],
                                         float (*sb)[S * S]) {
  const size_t img = (size_t)n * p.H * p.W;
  for (int i = threadIdx.x; i < S * S; i += SL_THREADS) {
    const int r = i / S, c = i - r * S, y = sy + r, x = sx + c;
    const bool in = y >= 0 && y < p.H && x >= 0 && x < p.W;
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
    if (in) {
      u = p.a[img + (size_t)y * p.W + x];
      v = p.b[img + (size_t)y * p.W + x];
    }
    sa[0][i] = in ? u.x - ka[0] : 0.f;
    sa[1][i] = in ? u.y - ka[1] : 0.f;
    sa[2][i] = in ? u.z - ka[2] : 0.f;
    sb[0][i] = in ? v.x - kb[0] : 0.f;
    sb[1][i] = in ? v.y - kb[1] : 0.f;
    sb[2][i] = in ? v.z - kb[2] : 0.f;
  }
}

// vertical pass of one channel: vm[moment][row r < NP][col c < NP + 10], moments a', b', a'^2, b'^2, a' b'
template <int NP, class P>
__device__ __forceinline__ void sl_vertical(const P& p, const float* sa, const float* sb, double* vm) {
  constexpr int S = NP + SL_HALO;
  for (int i = threadIdx.x; i < NP * S; i += SL_THREADS) {
    const int r = i / S, c = i - r * S;
    double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
    for (int k = 0; k < SL_WIN; ++k) {
      const double w = (double)p.w[k], u = (double)sa[(r + k) * S + c], v = (double)sb[(r + k) * S + c];
      const double wu = w * u, wv = w * v;
      a += wu; b += wv; aa += wu * u; bb += wv * v; ab += wu * v;
    }
    vm[0 * NP * S + i] = a; vm[1 * NP * S + i] = b; vm[2 * NP * S + i] = aa; vm[3 * NP * S + i] = bb; vm[4 * NP * S + i] = ab;
  }
}

template <int NP, class P>
__device__ __forceinline__ void sl_horizontal(const P& p, const double* vm, int r, int c, double* m) {
  constexpr int S = NP + SL_HALO;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SL_WIN; ++k) s += (double)p.w[k] * vm[q * NP * S + r * S + c + k];
    m[q] = s;
  }
}

// S and its coefficients at one position from the shifted moments md and the shifts.  The moments are summed in double and the
// three differences that cancel (the variances, the covariance, mu_b - mu_a) are taken in double: the shift cannot help where
// the image is steep under one window (a ramp across an 11-pixel image: E[a'^2] is ten times the variance whatever the shift),
// and fp32 moments there cost a digit on the loss and the gradient.  Everything after the differences is fp32.
__device__ __forceinline__ void sl_point(const double* md, float ka, float kb, float& S, float& A, float& B, float& C) {
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float sa2 = (float)(md[2] - md[0] * md[0]), sb2 = (float)(md[3] - md[1] * md[1]), sab = (float)(md[4] - md[0] * md[1]);
  const float m[2] = {(float)md[0], (float)md[1]};
  const float dm = (float)((md[1] - md[0]) + ((double)kb - (double)ka));
  const float mua = (float)(md[0] + (double)ka), mub = (float)(md[1] + (double)kb);
  const float N1 = 2.f * mua * mub + C1, D1 = mua * mua + mub * mub + C1, N2 = 2.f * sab + C2, D2 = sa2 + sb2 + C2;
  const float rD = 1.f / (D1 * D2);
  S = N1 * N2 * rD;
  B = -S / D2;
  C = 2.f * N1 * rD;
  const float dmu = 2.f * dm * (mub * (mua + mub) + C1) * N2 * rD / D1;
  A = dmu - 2.f * m[0] * B - m[1] * C;
}

// The contrast-structure part alone, cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2), and its coefficients about the same shift:
// B = dcs/ds_a^2 = -cs / D2, C = dcs/ds_ab = 2 / D2; the means enter through the moments only, A' = -2 mu_a' B - mu_b' C.
__device__ __forceinline__ void sl_point_cs(const double* md, float& S, float& A, float& B, float& C) {
  const float C2 = 0.03f * 0.03f;
  const float sa2 = (float)(md[2] - md[0] * md[0]), sb2 = (float)(md[3] - md[1] * md[1]), sab = (float)(md[4] - md[0] * md[1]);
  const float D2 = sa2 + sb2 + C2;
  S = (2.f * sab + C2) / D2;
  B = -S / D2;
  C = 2.f / D2;
  A = -2.f * (float)md[0] * B - (float)md[1] * C;
}

// the window, normalised to sum 1 in double
static inline void sl_window(float* w) {
  double g[SL_WIN], sum = 0.0;
  for (int k = 0; k < SL_WIN; ++k) {
    const double d = k - (SL_WIN - 1) / 2;
    g[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  for (int k = 0; k < SL_WIN; ++k) w[k] = (float)(g[k] / sum);
}
