// Image-quality metrics and the display conversion of the evaluator (test.py): per-image L1, MSE, PSNR and SSIM of a network
// output against its target, and the pitch-4 batch -> contiguous HWC images the figures and PNGs are made from.
//
// Metrics (new: the reference compares its models by eye only), per image, in fp32, on the output clamped to [0, 1] (what the
// reference displays, test.py:317-324) against the target as given, over the 3 logical channels of an S x S image:
//   l1   = mean |o - t|,  mse = mean (o - t)^2  over S*S*3 values,  psnr = 10 log10(1 / mse)  (+inf for mse == 0);
//   ssim = Wang, Bovik, Sheikh & Simoncelli (2004): 11 x 11 Gaussian window, sigma 1.5, normalised to sum 1; "valid" window
//          positions only ((S - 10)^2, no padding); C1 = 0.01^2, C2 = 0.03^2 (data range 1); population moments; averaged over
//          the positions and the 3 channels.
//
// k_image_metrics: one workgroup per 16 x 16 tile of an image's pixels.  It stages the tile plus the 10-pixel halo to its right
// and below (the windows whose top-left corner lies in the tile) of both images in LDS — one float4 load per pixel, all three
// channels together — then a vertical Gaussian pass and a horizontal one give the five moments (mu_o, mu_t, o^2, t^2, o t) of
// every window position of the tile; the same pass sums |o - t| and (o - t)^2 over the tile's own pixels.  Moments are taken
// about a per-tile, per-channel shift k (the tile's first pixel): sigma^2 = E[(o - k)^2] - E[o - k]^2 cancels far less than
// E[o^2] - mu^2 where the window is nearly flat, which is where C2 = 9e-4 makes SSIM sensitive to it (a constant image gives
// sigma = 0 exactly).  Each workgroup stores its three partial sums to its own workspace slot; k_metrics_final (one workgroup
// per image) sums an image's slots in a fixed order.  No float atomics: an image's metrics are the same bits whatever batch it
// is part of and however often it is evaluated.
//
// 8 x 256^2 pairs read ~16 MB once (the halo re-reads hit L2): launch-bound, tens of microseconds; written for clarity.
#include <math.h>

#include "vcg_common.h"

#define MT_TILE 16                        // window positions / own pixels per tile side
#define MT_WIN 11
#define MT_STAGE (MT_TILE + MT_WIN - 1)   // 26: staged pixels per side
#define MT_THREADS (MT_TILE * MT_TILE)

struct MetricsP {
  const float4* out;     // (N, Hp, Wp, 4) fp32, channel 3 unused; the images are the windows (top, left, H, W) of the buffers
  const float4* tgt;
  float* ws;             // [N][tiles][4] partial sums: l1, squared error, ssim (channel-averaged), 0
  float* res;            // [N][4]: l1, mse, psnr, ssim
  int H, W, Hp, Wp, top, left;
  int tiles_x, tiles_y;  // tiles per image = tiles_x * tiles_y, counted from the window's corner
  float w[MT_WIN];       // the Gaussian window, normalised in double on the host
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__global__ __launch_bounds__(MT_THREADS) void k_image_metrics(MetricsP p) {
  __shared__ float so[3][MT_STAGE * MT_STAGE], st[3][MT_STAGE * MT_STAGE];   // shifted pixels, by channel
  __shared__ float vm[15][MT_TILE * MT_STAGE];                                // vertical pass: [moment * 3 + channel][row][col]
  __shared__ float red[3][MT_THREADS];
  const int H = p.H, W = p.W, S = p.Wp, tid = threadIdx.x;            // S: the row pitch in pixels
  const int n = blockIdx.z, y0 = blockIdx.y * MT_TILE, x0 = blockIdx.x * MT_TILE;
  const size_t img = ((size_t)n * p.Hp + p.top) * p.Wp + p.left;    // the window's first pixel: nothing outside it is read
  const float4 ko4 = p.out[img + (size_t)y0 * S + x0], kt4 = p.tgt[img + (size_t)y0 * S + x0];
  const float ko[3] = {clamp01(ko4.x), clamp01(ko4.y), clamp01(ko4.z)}, kt[3] = {kt4.x, kt4.y, kt4.z};

  for (int i = tid; i < MT_STAGE * MT_STAGE; i += MT_THREADS) {
    const int r = i / MT_STAGE, c = i - r * MT_STAGE, y = y0 + r, x = x0 + c;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f), t = o;
    bool in = y < H && x < W;              // outside the image: only windows that are not valid read these
    if (in) {
      o = p.out[img + (size_t)y * S + x];
      t = p.tgt[img + (size_t)y * S + x];
    }
    so[0][i] = in ? clamp01(o.x) - ko[0] : 0.f;
    so[1][i] = in ? clamp01(o.y) - ko[1] : 0.f;
    so[2][i] = in ? clamp01(o.z) - ko[2] : 0.f;
    st[0][i] = in ? t.x - kt[0] : 0.f;
    st[1][i] = in ? t.y - kt[1] : 0.f;
    st[2][i] = in ? t.z - kt[2] : 0.f;
  }
  __syncthreads();

  // vertical pass: rows r of the tile, all MT_STAGE staged columns
  for (int i = tid; i < MT_TILE * MT_STAGE; i += MT_THREADS) {
    const int r = i / MT_STAGE, c = i - r * MT_STAGE;
    for (int ch = 0; ch < 3; ++ch) {
      float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
      for (int k = 0; k < MT_WIN; ++k) {
        const float w = p.w[k], u = so[ch][(r + k) * MT_STAGE + c], v = st[ch][(r + k) * MT_STAGE + c];
        a += w * u; b += w * v; aa += w * u * u; bb += w * v * v; ab += w * u * v;
      }
      vm[0 + ch][i] = a; vm[3 + ch][i] = b; vm[6 + ch][i] = aa; vm[9 + ch][i] = bb; vm[12 + ch][i] = ab;
    }
  }
  __syncthreads();

  // horizontal pass + SSIM at this thread's window position; L1 / squared error of its own pixel
  const int r = tid / MT_TILE, c = tid - r * MT_TILE, y = y0 + r, x = x0 + c;
  float ssim = 0.f, l1 = 0.f, se = 0.f;
  if (y < H - (MT_WIN - 1) && x < W - (MT_WIN - 1)) {
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    for (int ch = 0; ch < 3; ++ch) {
      float m[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MT_WIN; ++k) s += p.w[k] * vm[q * 3 + ch][r * MT_STAGE + c + k];
        m[q] = s;
      }
      const float so2 = m[2] - m[0] * m[0], st2 = m[3] - m[1] * m[1], sot = m[4] - m[0] * m[1];
      const float mo = m[0] + ko[ch], mt = m[1] + kt[ch];
      ssim += ((2.f * mo * mt + C1) * (2.f * sot + C2)) / ((mo * mo + mt * mt + C1) * (so2 + st2 + C2));
    }
    ssim *= (1.f / 3.f);
  }
  if (y < H && x < W) {
    const float4 o = p.out[img + (size_t)y * S + x], t = p.tgt[img + (size_t)y * S + x];
    const float d0 = clamp01(o.x) - t.x, d1 = clamp01(o.y) - t.y, d2 = clamp01(o.z) - t.z;
    l1 = fabsf(d0) + fabsf(d1) + fabsf(d2);
    se = d0 * d0 + d1 * d1 + d2 * d2;
  }

  red[0][tid] = l1; red[1][tid] = se; red[2][tid] = ssim;
  __syncthreads();
  for (int h = MT_THREADS / 2; h > 0; h >>= 1) {   // fixed-order tree
    if (tid < h) {
      red[0][tid] += red[0][tid + h];
      red[1][tid] += red[1][tid + h];
      red[2][tid] += red[2][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float* slot = p.ws + ((size_t)n * p.tiles_x * p.tiles_y + (size_t)blockIdx.y * p.tiles_x + blockIdx.x) * 4;
    slot[0] = red[0][0]; slot[1] = red[1][0]; slot[2] = red[2][0]; slot[3] = 0.f;
  }
}

__global__ __launch_bounds__(256) void k_metrics_final(MetricsP p) {
  __shared__ float red[3][256];
  const int n = blockIdx.x, tid = threadIdx.x, tiles = p.tiles_x * p.tiles_y;
  const float* ws = p.ws + (size_t)n * tiles * 4;
  float a = 0.f, b = 0.f, c = 0.f;
  for (int i = tid; i < tiles; i += 256) {          // each thread a fixed strided subset, in order
    a += ws[i * 4 + 0]; b += ws[i * 4 + 1]; c += ws[i * 4 + 2];
  }
  red[0][tid] = a; red[1][tid] = b; red[2][tid] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      red[0][tid] += red[0][tid + h];
      red[1][tid] += red[1][tid + h];
      red[2][tid] += red[2][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float npx = 3.f * (float)p.H * (float)p.W, nwin = (float)(p.H - (MT_WIN - 1)) * (float)(p.W - (MT_WIN - 1));
    const float mse = red[1][0] / npx;
    float* o = p.res + (size_t)n * 4;
    o[0] = red[0][0] / npx;
    o[1] = mse;
    o[2] = mse > 0.f ? 10.f * log10f(1.f / mse) : INFINITY;
    o[3] = red[2][0] / nwin;
  }
}

// both entry points: the window (top, left, H, W) of two (N, Hp, Wp, 4) buffers
static int metrics_launch(const char* who, const float* out, const float* target, float* result, int N, int Hp, int Wp, int top,
                          int left, int H, int W, float* ws, size_t ws_bytes, void* stream) {
  MetricsP p;
  p.out = (const float4*)out; p.tgt = (const float4*)target; p.ws = ws; p.res = result;
  p.H = H; p.W = W; p.Hp = Hp; p.Wp = Wp; p.top = top; p.left = left;
  p.tiles_x = (W + MT_TILE - 1) / MT_TILE;
  p.tiles_y = (H + MT_TILE - 1) / MT_TILE;
  const size_t need = (size_t)N * p.tiles_x * p.tiles_y * 4 * sizeof(float);
  VCG_CHECK_ARG(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
  double g[MT_WIN], sum = 0.0;
  for (int k = 0; k < MT_WIN; ++k) {
    const double d = k - (MT_WIN - 1) / 2;
    g[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  for (int k = 0; k < MT_WIN; ++k) p.w[k] = (float)(g[k] / sum);
  hipLaunchKernelGGL(k_image_metrics, dim3(p.tiles_x, p.tiles_y, N), dim3(MT_THREADS), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(k_metrics_final, dim3(N), dim3(256), 0, (hipStream_t)stream, p);
  VCG_LAUNCH_CHECK(who);
  return 0;
}

extern "C" int vcg_image_metrics(const float* out, const float* target, float* result, int N, int S, float* ws, size_t ws_bytes,
                                 void* stream) {
  VCG_CHECK_ARG(out && target && result && ws, "vcg_image_metrics: null pointer");
  VCG_CHECK_ARG(N > 0 && S >= MT_WIN && S <= 4096, "vcg_image_metrics: bad N=%d S=%d (SSIM's 11x11 window needs S >= 11)", N, S);
  return metrics_launch("vcg_image_metrics", out, target, result, N, S, S, 0, 0, S, S, ws, ws_bytes, stream);
}

extern "C" int vcg_image_metrics_hw(const float* out, const float* target, float* result, int N, int Hp, int Wp, int top, int left,
                                    int H, int W, float* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(out && target && result && ws, "vcg_image_metrics_hw: null pointer");
  VCG_CHECK_ARG(N > 0 && N <= 65535 && H >= MT_WIN && W >= MT_WIN && Hp <= 65535 && Wp <= 65535,
                "vcg_image_metrics_hw: bad N=%d H=%d W=%d (SSIM's 11x11 window needs H, W >= 11)", N, H, W);
  VCG_CHECK_ARG(top >= 0 && left >= 0 && top + H <= Hp && left + W <= Wp,
                "vcg_image_metrics_hw: the %dx%d window at (%d, %d) leaves the %dx%d buffer", H, W, top, left, Hp, Wp);
  return metrics_launch("vcg_image_metrics_hw", out, target, result, N, Hp, Wp, top, left, H, W, ws, ws_bytes, stream);
}

// pitch-4 fp32 (N, S, S, 4) -> contiguous (N, S, S, 3): fp32 clamped to [0, 1], or uint8 floor(255 v + 0.5) clipped to 0..255
// (input.hip's u8_of rule, evaluated in double so that it is the exact floor, not that of a rounded or fused 255 v + 0.5)
__global__ __launch_bounds__(256) void k_to_display(const float4* __restrict__ x, void* __restrict__ out, size_t npx, int as_u8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
    const float4 v = x[i];
    const float c[3] = {v.x, v.y, v.z};
    if (as_u8) {
      unsigned char* o = (unsigned char*)out + 3 * i;
      for (int k = 0; k < 3; ++k) {
        const double q = floor(255.0 * (double)c[k] + 0.5);
        o[k] = (unsigned char)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
      }
    } else {
      float* o = (float*)out + 3 * i;
      for (int k = 0; k < 3; ++k) o[k] = clamp01(c[k]);
    }
  }
}

extern "C" int vcg_to_display(const float* x, void* out, int N, int S, int as_uint8, void* stream) {
  VCG_CHECK_ARG(x && out, "vcg_to_display: null pointer");
  VCG_CHECK_ARG(N > 0 && S > 0 && S <= 4096, "vcg_to_display: bad N=%d S=%d", N, S);
  const size_t npx = (size_t)N * S * S;
  size_t blocks = (npx + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(k_to_display, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)x, out, npx,
                     as_uint8 ? 1 : 0);
  VCG_LAUNCH_CHECK("vcg_to_display");
  return 0;
}
