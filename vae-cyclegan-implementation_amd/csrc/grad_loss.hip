// Multi-scale gradient-matching loss (Eigen & Fergus 2015; Li & Snavely 2018): an L1 on the horizontal and vertical finite
// differences of d = generated - target, taken at S = `scales` subsampled scales, forward and the gradient with respect to the
// generated image.  Operands are (N, H, W, 4) fp32, channel 3 is padding and never enters a sum.  H, W >= 1, S in 1..4.
//
//   d_s[i, j] = d[i 2^s, j 2^s],   H_s = ceil(H / 2^s),   W_s = ceil(W / 2^s),   s = 0 .. S - 1
//   X_s = sum |d_s[i, j+1] - d_s[i, j]|  over n, c in {0, 1, 2}, i < H_s, j < W_s - 1       M_sx = 3 N H_s (W_s - 1)
//   Y_s = sum |d_s[i+1, j] - d_s[i, j]|  over n, c, i < H_s - 1, j < W_s                    M_sy = 3 N (H_s - 1) W_s
//   loss = 1 / S  sum_s (X_s / M_sx + Y_s / M_sy),   a direction with no pair (M = 0) contributes 0
//
// In pixel coordinates: the pixel (y, x) with 2^s | y and 2^s | x owns, at scale s, the pair with its right neighbour
// (y, x + 2^s) if x + 2^s < W and the pair with its lower neighbour (y + 2^s, x) if y + 2^s < H.
//
// k_grad_fwd<S>: one workgroup per 32 x 32 tile of pixels (the origin a multiple of 8 in both coordinates, so divisibility by
// 2^s is a property of the position inside the tile).  It reads a and b once, one float4 load per pixel, and stages d of the tile
// and of a halo of 2^(S-1) pixels to the right and below in LDS — as doubles: the difference of two floats is exact there, and
// so is the difference of two such differences, which leaves the two conversions to fp32 as the only roundings of the loss.  Each
// thread adds the pairs its pixels own into 2 S sums (X_s, Y_s), these go through a wavefront shuffle, then a block partial, into
// the tile's own 2 S slots of the workspace.  k_grad_final (one workgroup) adds the slots in a fixed order, applies 1 / (S M)
// and writes out[0].  No float atomics: the same input gives the same bits.
// k_grad_bwd<S>: one launch, no workspace, in gather form.  One workgroup per 32 x 32 tile of pixels stages d (fp32: only its
// signs are used) with the halo on all four sides; every pixel sums the up to 4 S sign terms of the pairs it belongs to,
//   ga(y, x) = gout sum over s with 2^s | y, 2^s | x of  [sgn(left pair) - sgn(right pair)] / (S M_sx) + [sgn(upper) - sgn(lower)] / (S M_sy),
// sgn(0) = 0 (torch's abs), pairs that do not exist dropped.  ga is written for every pixel, channel 3 = 0.
#include "vcg_common.h"

#define GL_TILE 32
#define GL_THREADS 256
#define GL_MAX_SCALES 4

struct GradP {
  const float4* a;       // generated, (N, H, W, 4)
  const float4* b;       // target
  double* slots;         // [N * tiles_y * tiles_x][2 S]: X_0, Y_0, X_1, Y_1, ... of each tile
  float* out;            // out[0] = the loss
  const float* gout;     // gout[0], read on the device
  float4* ga;            // (N, H, W, 4)
  int H, W, S, ntiles;
  double cx[GL_MAX_SCALES], cy[GL_MAX_SCALES];     // 1 / (S M_sx), 1 / (S M_sy); 0 where M = 0
  float fx[GL_MAX_SCALES], fy[GL_MAX_SCALES];      // the same in fp32 (backward)
};

template <int S>
__global__ __launch_bounds__(GL_THREADS) void k_grad_fwd(GradP p) {
  constexpr int HALO = 1 << (S - 1), SW = GL_TILE + HALO;
  __shared__ double sd[3][SW * SW];
  __shared__ double red[GL_THREADS / VCG_WAVE][2 * S];
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * GL_TILE, x0 = blockIdx.x * GL_TILE;
  const size_t img = (size_t)n * p.H * p.W;
  // d of the pixels (y0 + r, x0 + c), r, c < SW; outside the image 0 (never read: a pair exists only inside the image)
  for (int i = tid; i < SW * SW; i += GL_THREADS) {
    const int r = i / SW, c = i - r * SW, y = y0 + r, x = x0 + c;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (y < p.H && x < p.W) {
      const float4 u = p.a[img + (size_t)y * p.W + x], v = p.b[img + (size_t)y * p.W + x];
      d0 = (double)u.x - (double)v.x;
      d1 = (double)u.y - (double)v.y;
      d2 = (double)u.z - (double)v.z;
    }
    sd[0][i] = d0; sd[1][i] = d1; sd[2][i] = d2;
  }
  __syncthreads();
  double acc[2 * S];
#pragma unroll
  for (int q = 0; q < 2 * S; ++q) acc[q] = 0.0;
  for (int i = tid; i < GL_TILE * GL_TILE; i += GL_THREADS) {
    const int r = i / GL_TILE, c = i - r * GL_TILE, y = y0 + r, x = x0 + c;
    if (y < p.H && x < p.W) {
      const int o = r * SW + c;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int st = 1 << s;                       // c + st, r + st <= GL_TILE - 1 + HALO = SW - 1
        if (((r | c) & (st - 1)) == 0) {
          if (x + st < p.W)
            acc[2 * s] += fabs(sd[0][o + st] - sd[0][o]) + fabs(sd[1][o + st] - sd[1][o]) + fabs(sd[2][o + st] - sd[2][o]);
          if (y + st < p.H)
            acc[2 * s + 1] += fabs(sd[0][o + st * SW] - sd[0][o]) + fabs(sd[1][o + st * SW] - sd[1][o]) +
                              fabs(sd[2][o + st * SW] - sd[2][o]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 2 * S; ++q) {
    const double w = wave_sum_d(acc[q]);
    if ((tid & (VCG_WAVE - 1)) == 0) red[tid / VCG_WAVE][q] = w;
  }
  __syncthreads();
  if (tid < 2 * S) {
    double t = red[0][tid];
    for (int w = 1; w < GL_THREADS / VCG_WAVE; ++w) t += red[w][tid];        // fixed order
    const size_t tile = ((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    p.slots[tile * (2 * S) + tid] = t;
  }
}

// 32 groups of 8 threads: thread (g, q) adds quantity q (X_0, Y_0, X_1, ...) of the tiles g, g + 32, ... in order
__global__ __launch_bounds__(256) void k_grad_final(GradP p) {
  __shared__ double red[256];
  const int tid = threadIdx.x, q = tid & 7, g = tid >> 3;
  double s = 0.0;
  if (q < 2 * p.S)
    for (int t = g; t < p.ntiles; t += 32) s += p.slots[(size_t)t * (2 * p.S) + q];
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h >= 8; h >>= 1) {             // a multiple of 8 apart: the quantities stay apart
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    double loss = 0.0;
    for (int k = 0; k < p.S; ++k) loss += red[2 * k] * p.cx[k] + red[2 * k + 1] * p.cy[k];
    p.out[0] = (float)loss;
  }
}

__device__ __forceinline__ float gl_sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }

template <int S>
__global__ __launch_bounds__(GL_THREADS) void k_grad_bwd(GradP p) {
  constexpr int HALO = 1 << (S - 1), SW = GL_TILE + 2 * HALO;
  __shared__ float sd[3][SW * SW];
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * GL_TILE, x0 = blockIdx.x * GL_TILE;
  const size_t img = (size_t)n * p.H * p.W;
  // d of the pixels (y0 - HALO + r, x0 - HALO + c), r, c < SW; outside the image 0 (never read)
  for (int i = tid; i < SW * SW; i += GL_THREADS) {
    const int r = i / SW, c = i - r * SW, y = y0 - HALO + r, x = x0 - HALO + c;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
      const float4 u = p.a[img + (size_t)y * p.W + x], v = p.b[img + (size_t)y * p.W + x];
      d0 = u.x - v.x; d1 = u.y - v.y; d2 = u.z - v.z;
    }
    sd[0][i] = d0; sd[1][i] = d1; sd[2][i] = d2;
  }
  __syncthreads();
  const float go = p.gout[0];
  for (int i = tid; i < GL_TILE * GL_TILE; i += GL_THREADS) {
    const int r = i / GL_TILE, c = i - r * GL_TILE, y = y0 + r, x = x0 + c;
    if (y >= p.H || x >= p.W) continue;
    const int o = (r + HALO) * SW + c + HALO;
    float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int st = 1 << s;
      if (((r | c) & (st - 1)) != 0) continue;
      const bool L = x - st >= 0, R = x + st < p.W, U = y - st >= 0, D = y + st < p.H;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float v = sd[ch][o];
        const float tx = (L ? gl_sgn(v - sd[ch][o - st]) : 0.f) - (R ? gl_sgn(sd[ch][o + st] - v) : 0.f);
        const float ty = (U ? gl_sgn(v - sd[ch][o - st * SW]) : 0.f) - (D ? gl_sgn(sd[ch][o + st * SW] - v) : 0.f);
        g[ch] += p.fx[s] * tx + p.fy[s] * ty;
      }
    }
    p.ga[img + (size_t)y * p.W + x] = make_float4(go * g[0], go * g[1], go * g[2], 0.f);
  }
}

static int gl_args(const char* who, int N, int H, int W, int scales) {
  VCG_CHECK_ARG(N > 0 && N <= 65535, "%s: bad N=%d", who, N);
  VCG_CHECK_ARG(H > 0 && W > 0, "%s: bad H=%d W=%d", who, H, W);
  VCG_CHECK_ARG(H <= 32768 && W <= 32768, "%s: H=%d W=%d above 32768", who, H, W);
  VCG_CHECK_ARG(scales >= 1 && scales <= GL_MAX_SCALES, "%s: bad scales=%d (1 .. %d)", who, scales, GL_MAX_SCALES);
  return 0;
}

static size_t gl_tiles(int N, int H, int W) {
  return (size_t)N * ((H + GL_TILE - 1) / GL_TILE) * ((W + GL_TILE - 1) / GL_TILE);
}

static void gl_fill(GradP& p, int N, int H, int W, int S) {
  p.H = H; p.W = W; p.S = S;
  p.ntiles = (int)gl_tiles(N, H, W);
  for (int s = 0; s < S; ++s) {
    const double hs = (double)((H + (1 << s) - 1) >> s), ws = (double)((W + (1 << s) - 1) >> s);
    const double mx = 3.0 * N * hs * (ws - 1.0), my = 3.0 * N * (hs - 1.0) * ws;
    p.cx[s] = mx > 0.0 ? 1.0 / (S * mx) : 0.0;
    p.cy[s] = my > 0.0 ? 1.0 / (S * my) : 0.0;
    p.fx[s] = (float)p.cx[s];
    p.fy[s] = (float)p.cy[s];
  }
}

extern "C" size_t vcg_grad_loss_workspace(int N, int H, int W, int scales) {
  if (gl_args("vcg_grad_loss_workspace", N, H, W, scales) != 0) return 0;
  const size_t tiles = gl_tiles(N, H, W);
  if (tiles > 0x7FFFFFFFu) {
    vcg_set_error("vcg_grad_loss_workspace: N=%d H=%d W=%d has too many tiles", N, H, W);
    return 0;
  }
  return (tiles * 2 * scales * sizeof(double) + 15) / 16 * 16;
}

extern "C" int vcg_grad_loss_fwd(const float* a, const float* b, float* out, int N, int H, int W, int scales, void* ws,
                                 size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(a && b && out && ws, "vcg_grad_loss_fwd: null pointer");
  if (gl_args("vcg_grad_loss_fwd", N, H, W, scales) != 0) return -1;
  const size_t need = vcg_grad_loss_workspace(N, H, W, scales);
  VCG_CHECK_ARG(need != 0, "vcg_grad_loss_fwd: N=%d H=%d W=%d has too many tiles", N, H, W);
  VCG_CHECK_ARG(ws_bytes >= need, "vcg_grad_loss_fwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_grad_loss_fwd: workspace not 16-byte aligned");
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "vcg_grad_loss_fwd: images not 16-byte aligned");
  GradP p;
  memset(&p, 0, sizeof(p));
  p.a = (const float4*)a; p.b = (const float4*)b; p.slots = (double*)ws; p.out = out;
  gl_fill(p, N, H, W, scales);
  const dim3 grid((W + GL_TILE - 1) / GL_TILE, (H + GL_TILE - 1) / GL_TILE, N), block(GL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (scales) {
    case 1: hipLaunchKernelGGL(k_grad_fwd<1>, grid, block, 0, st, p); break;
    case 2: hipLaunchKernelGGL(k_grad_fwd<2>, grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL(k_grad_fwd<3>, grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL(k_grad_fwd<4>, grid, block, 0, st, p); break;
  }
  hipLaunchKernelGGL(k_grad_final, dim3(1), dim3(256), 0, st, p);
  VCG_LAUNCH_CHECK("vcg_grad_loss_fwd");
  return 0;
}

extern "C" int vcg_grad_loss_bwd(const float* a, const float* b, const float* gout, float* ga, int N, int H, int W, int scales,
                                 void* stream) {
  VCG_CHECK_ARG(a && b && gout && ga, "vcg_grad_loss_bwd: null pointer");
  if (gl_args("vcg_grad_loss_bwd", N, H, W, scales) != 0) return -1;
  VCG_CHECK_ARG(gl_tiles(N, H, W) <= 0x7FFFFFFFu, "vcg_grad_loss_bwd: N=%d H=%d W=%d has too many tiles", N, H, W);
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)ga) & 15) == 0, "vcg_grad_loss_bwd: images not 16-byte aligned");
  GradP p;
  memset(&p, 0, sizeof(p));
  p.a = (const float4*)a; p.b = (const float4*)b; p.gout = gout; p.ga = (float4*)ga;
  gl_fill(p, N, H, W, scales);
  const dim3 grid((W + GL_TILE - 1) / GL_TILE, (H + GL_TILE - 1) / GL_TILE, N), block(GL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (scales) {
    case 1: hipLaunchKernelGGL(k_grad_bwd<1>, grid, block, 0, st, p); break;
    case 2: hipLaunchKernelGGL(k_grad_bwd<2>, grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL(k_grad_bwd<3>, grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL(k_grad_bwd<4>, grid, block, 0, st, p); break;
  }
  VCG_LAUNCH_CHECK("vcg_grad_loss_bwd");
  return 0;
}
