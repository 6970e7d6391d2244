// Structural training loss: 1 - SSIM of a generated image against its target, forward and the gradient with respect to the
// generated image.  Definition of csrc/metrics.hip (11 x 11 Gaussian window, sigma 1.5, normalised to sum 1 in double on the host;
// "valid" positions only, (H - 10) x (W - 10); C1 = 0.01^2, C2 = 0.03^2; population moments) WITHOUT the clamp of the generated
// image: the gradient must exist everywhere.  Operands are (N, H, W, 4) fp32, channel 3 is padding and never enters a sum.
//
//   loss = 1 - 1 / M  sum over (n, c in {0, 1, 2}, valid positions p) of S(p),      M = 3 N (H - 10) (W - 10)
//   S = (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2))
//
// Backward.  With B = dS/ds_a^2 = -S / D2, C = dS/ds_ab = 2 N1 / (D1 D2) and A = dS/dmu_a - 2 mu_a B - mu_b C per position,
//   ga(q) = -gout / M [ (w * A)(q) + 2 a(q) (w * B)(q) + b(q) (w * C)(q) ],
// * the transposed ("full") separable filter over the valid positions.  All of it is evaluated about a per-tile, per-channel
// shift k (the tile's first pixel, as in metrics.hip): a' = a - k_a, b' = b - k_b leave the variances alone, and
//   ga(q) = -gout / M [ (w * A')(q) + 2 a'(q) (w * B)(q) + b'(q) (w * C)(q) ],   A' = dS/dmu_a - 2 mu_a' B - mu_b' C,
// where the terms 2 a' B and 2 mu_a' B, which cancel to 2 B (a - mu_a) with B up to 1 / C2 = 1100, are both small instead of both
// of order B.  dS/dmu_a is taken in its factored form 2 (mu_b - mu_a)(mu_b (mu_a + mu_b) + C1) N2 / (D1^2 D2).
//
// k_ssim_fwd: one workgroup per 16 x 16 tile of window positions; stages the 26 x 26 pixels under them (both images, three
// channels, one float4 load per pixel), vertical then horizontal 11-tap pass per channel with the five moments summed in double
// (sl_point says why), sums S over its valid positions in double and stores the partial to a slot of its own.  k_ssim_final (one
// workgroup) sums the slots in a fixed order.  No float atomics: the same input gives the same bits.
// k_ssim_bwd: one workgroup per 16 x 16 tile of PIXELS.  The forward keeps nothing: the backward recomputes the coefficients of
// the 26 x 26 positions whose windows touch the tile from a 36 x 36 pixel stage (a 20-pixel halo, one channel at a time), then
// runs the transposed passes over them.  A, B, C of a position are only meaningful together with the shift they were taken
// about, and a pixel receives from positions of up to four forward tiles: recomputing under ONE shift per backward tile keeps
// the sum free of that cancellation, which a workspace of coefficients written under the forward's shifts would not (DESIGN.md,
// "The structural loss").  ga is written for every pixel, channel 3 = 0.
#include <math.h>

#include "ssim_window.h"
#include "vcg_common.h"

struct SsimP {
  const float4* a;       // generated, (N, H, W, 4)
  const float4* b;       // target
  double* slots;         // [N * tiles_y * tiles_x] partial sums of S
  float* out;            // out[0] = the loss
  const float* gout;     // gout[0], read on the device
  float4* ga;            // (N, H, W, 4)
  int H, W, tiles_x, tiles_y, nslots;
  double inv_m;          // 1 / M
  float w[SL_WIN];
};

__global__ __launch_bounds__(SL_THREADS) void k_ssim_fwd(SsimP p) {
  __shared__ float sa[3][SL_FS * SL_FS], sb[3][SL_FS * SL_FS];
  __shared__ double vm[5 * SL_FP * SL_FS];
  __shared__ double red[SL_THREADS];
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * SL_FP, x0 = blockIdx.x * SL_FP;
  const size_t first = ((size_t)n * p.H + y0) * p.W + x0;           // a valid position: inside the image
  const float4 ka4 = p.a[first], kb4 = p.b[first];
  const float ka[3] = {ka4.x, ka4.y, ka4.z}, kb[3] = {kb4.x, kb4.y, kb4.z};
  sl_stage<SL_FS>(p, n, y0, x0, ka, kb, sa, sb);
  __syncthreads();
  const int r = tid / SL_FP, c = tid - r * SL_FP;
  const bool valid = y0 + r < p.H - SL_HALO && x0 + c < p.W - SL_HALO;
  float ssim = 0.f;
  for (int ch = 0; ch < 3; ++ch) {
    sl_vertical<SL_FP>(p, sa[ch], sb[ch], vm);
    __syncthreads();
    if (valid) {
      double m[5];
      float S, A, B, C;
      sl_horizontal<SL_FP>(p, vm, r, c, m);
      sl_point(m, ka[ch], kb[ch], S, A, B, C);
      ssim += S;
    }
    __syncthreads();
  }
  red[tid] = (double)ssim;
  __syncthreads();
  for (int h = SL_THREADS / 2; h > 0; h >>= 1) {   // fixed-order tree
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) p.slots[((size_t)n * p.tiles_y + blockIdx.y) * p.tiles_x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_ssim_final(SsimP p) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < p.nslots; i += 256) s += p.slots[i];          // each thread a fixed strided subset, in order
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) p.out[0] = (float)(1.0 - red[0] * p.inv_m);
}

__global__ __launch_bounds__(SL_THREADS) void k_ssim_bwd(SsimP p) {
  __shared__ float sa[SL_BS * SL_BS], sb[SL_BS * SL_BS];              // one channel at a time: the double moments take the room
  __shared__ double vm[5 * SL_BP * SL_BS];                            // the transposed vertical pass reuses it (vt below)
  __shared__ float cf[3][SL_BP * SL_BP];                              // A', B, C of the positions; 0 where a position is not valid
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * SL_TILE, x0 = blockIdx.x * SL_TILE;
  const size_t first = ((size_t)n * p.H + y0) * p.W + x0;           // the tile's first pixel: inside the image
  const float4 ka4 = p.a[first], kb4 = p.b[first];
  const float ka[3] = {ka4.x, ka4.y, ka4.z}, kb[3] = {kb4.x, kb4.y, kb4.z};
  const int py0 = y0 - SL_HALO, px0 = x0 - SL_HALO;                  // first position / first staged pixel
  const float scale = -p.gout[0] * (float)p.inv_m;
  const int r = tid / SL_TILE, c = tid - r * SL_TILE;
  float* vt = (float*)vm;                                             // [3][SL_TILE][SL_BP]
  float g[3];
  for (int ch = 0; ch < 3; ++ch) {
    // pixels (py0 + r, px0 + c) of channel ch minus the shift; outside the image 0 (read by positions that are not valid only)
    for (int i = tid; i < SL_BS * SL_BS; i += SL_THREADS) {
      const int sr = i / SL_BS, sc = i - sr * SL_BS, y = py0 + sr, x = px0 + sc;
      float u = 0.f, v = 0.f;
      if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
        const float4 ua = p.a[((size_t)n * p.H + y) * p.W + x], vb = p.b[((size_t)n * p.H + y) * p.W + x];
        u = (ch == 0 ? ua.x : ch == 1 ? ua.y : ua.z) - ka[ch];
        v = (ch == 0 ? vb.x : ch == 1 ? vb.y : vb.z) - kb[ch];
      }
      sa[i] = u; sb[i] = v;
    }
    __syncthreads();
    sl_vertical<SL_BP>(p, sa, sb, vm);
    __syncthreads();
    for (int i = tid; i < SL_BP * SL_BP; i += SL_THREADS) {
      const int pr = i / SL_BP, pc = i - pr * SL_BP, py = py0 + pr, px = px0 + pc;
      float S, A = 0.f, B = 0.f, C = 0.f;
      if (py >= 0 && py < p.H - SL_HALO && px >= 0 && px < p.W - SL_HALO) {
        double m[5];
        sl_horizontal<SL_BP>(p, vm, pr, pc, m);
        sl_point(m, ka[ch], kb[ch], S, A, B, C);
      }
      cf[0][i] = A; cf[1][i] = B; cf[2][i] = C;
    }
    __syncthreads();
    // pixel row y0 + rr receives from position rows y0 + rr - k, k < 11: tile rows rr + 10 - k
    for (int i = tid; i < SL_TILE * SL_BP; i += SL_THREADS) {
      const int rr = i / SL_BP, cc = i - rr * SL_BP;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < SL_WIN; ++k) {
        const float w = p.w[k];
        const int j = (rr + SL_HALO - k) * SL_BP + cc;
        s0 += w * cf[0][j]; s1 += w * cf[1][j]; s2 += w * cf[2][j];
      }
      vt[0 * SL_TILE * SL_BP + i] = s0; vt[1 * SL_TILE * SL_BP + i] = s1; vt[2 * SL_TILE * SL_BP + i] = s2;
    }
    __syncthreads();
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
    for (int k = 0; k < SL_WIN; ++k) {
      const float w = p.w[k];
      const int j = r * SL_BP + c + SL_HALO - k;
      o0 += w * vt[0 * SL_TILE * SL_BP + j]; o1 += w * vt[1 * SL_TILE * SL_BP + j]; o2 += w * vt[2 * SL_TILE * SL_BP + j];
    }
    const int own = (r + SL_HALO) * SL_BS + c + SL_HALO;
    g[ch] = scale * (o0 + 2.f * sa[own] * o1 + sb[own] * o2);
    __syncthreads();
  }
  if (y0 + r < p.H && x0 + c < p.W) p.ga[((size_t)n * p.H + y0 + r) * p.W + x0 + c] = make_float4(g[0], g[1], g[2], 0.f);
}

static int sl_args(const char* who, int N, int H, int W) {
  VCG_CHECK_ARG(N > 0 && N <= 65535, "%s: bad N=%d", who, N);
  VCG_CHECK_ARG(H >= SL_WIN && W >= SL_WIN, "%s: bad H=%d W=%d (SSIM's 11x11 window needs H, W >= 11)", who, H, W);
  VCG_CHECK_ARG(H <= 32768 && W <= 32768, "%s: H=%d W=%d above 32768", who, H, W);
  return 0;
}

static void sl_fill(SsimP& p, int N, int H, int W) {
  p.H = H; p.W = W;
  p.tiles_x = (W - SL_HALO + SL_FP - 1) / SL_FP;
  p.tiles_y = (H - SL_HALO + SL_FP - 1) / SL_FP;
  p.nslots = N * p.tiles_x * p.tiles_y;
  p.inv_m = 1.0 / (3.0 * (double)N * (double)(H - SL_HALO) * (double)(W - SL_HALO));
  sl_window(p.w);
}

extern "C" size_t vcg_ssim_loss_workspace(int N, int H, int W) {
  if (sl_args("vcg_ssim_loss_workspace", N, H, W) != 0) return 0;
  const size_t tiles = (size_t)((W - SL_HALO + SL_FP - 1) / SL_FP) * ((H - SL_HALO + SL_FP - 1) / SL_FP);
  if ((size_t)N * tiles > 0x7FFFFFFFu) {
    vcg_set_error("vcg_ssim_loss_workspace: N=%d H=%d W=%d has too many tiles", N, H, W);
    return 0;
  }
  return ((size_t)N * tiles * sizeof(double) + 15) / 16 * 16;
}

extern "C" int vcg_ssim_loss_fwd(const float* a, const float* b, float* out, int N, int H, int W, void* ws, size_t ws_bytes,
                                 void* stream) {
  VCG_CHECK_ARG(a && b && out && ws, "vcg_ssim_loss_fwd: null pointer");
  if (sl_args("vcg_ssim_loss_fwd", N, H, W) != 0) return -1;
  const size_t need = vcg_ssim_loss_workspace(N, H, W);
  VCG_CHECK_ARG(need != 0, "vcg_ssim_loss_fwd: N=%d H=%d W=%d has too many tiles", N, H, W);
  VCG_CHECK_ARG(ws_bytes >= need, "vcg_ssim_loss_fwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_ssim_loss_fwd: workspace not 16-byte aligned");
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "vcg_ssim_loss_fwd: images not 16-byte aligned");
  SsimP p;
  memset(&p, 0, sizeof(p));
  p.a = (const float4*)a; p.b = (const float4*)b; p.slots = (double*)ws; p.out = out;
  sl_fill(p, N, H, W);
  hipLaunchKernelGGL(k_ssim_fwd, dim3(p.tiles_x, p.tiles_y, N), dim3(SL_THREADS), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(k_ssim_final, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
  VCG_LAUNCH_CHECK("vcg_ssim_loss_fwd");
  return 0;
}

extern "C" int vcg_ssim_loss_bwd(const float* a, const float* b, const float* gout, float* ga, int N, int H, int W, void* stream) {
  VCG_CHECK_ARG(a && b && gout && ga, "vcg_ssim_loss_bwd: null pointer");
  if (sl_args("vcg_ssim_loss_bwd", N, H, W) != 0) return -1;
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)ga) & 15) == 0, "vcg_ssim_loss_bwd: images not 16-byte aligned");
  SsimP p;
  memset(&p, 0, sizeof(p));
  p.a = (const float4*)a; p.b = (const float4*)b; p.gout = gout; p.ga = (float4*)ga;
  sl_fill(p, N, H, W);
  hipLaunchKernelGGL(k_ssim_bwd, dim3((W + SL_TILE - 1) / SL_TILE, (H + SL_TILE - 1) / SL_TILE, N), dim3(SL_THREADS), 0,
                     (hipStream_t)stream, p);
  VCG_LAUNCH_CHECK("vcg_ssim_loss_bwd");
  return 0;
}
