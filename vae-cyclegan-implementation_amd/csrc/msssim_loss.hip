// Multi-scale structural training loss (MS-SSIM; Wang, Simoncelli & Bovik 2003), forward and the gradient with respect to the
// generated image.  Window, constants and layout are those of ssim_loss.hip (ssim_window.h); operands (N, H, W, 4) fp32, channel 3
// never enters a sum.  K = `scales` levels: level 0 is the images, level j + 1 the 2 x 2 mean of level j at stride 2 with
// H_{j+1} = H_j / 2, W_{j+1} = W_j / 2 (a last odd row or column is dropped); min(H, W) >> (K - 1) >= 11.
//
//   f_j(n, c) = mean over level j's valid positions of cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2)    for j < K - 1,
//   f_{K-1}(n, c) = mean of the full S,
//   MS(n, c) = prod_j max(f_j, FLOOR)^{w_j},  FLOOR = 1e-4,  w = the first K of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) over
//   their sum (in double),   loss = 1 - mean over (n, c) of MS.
//
// Forward, per level: k_ms_pool writes both images' next level; k_ms_fwd is k_ssim_fwd with one partial sum per CHANNEL, to
// slots[n][c][tile].  k_ms_final (one workgroup) sums every (n, c, level)'s slots in a fixed order (a wave per sum, then a fixed
// butterfly), forms the products and the loss, and writes coef[n][c][j] = d loss / d f_j = -MS w_j / (3 N f_j), 0 where f_j was
// clamped (torch.clamp's gradient: a clamped factor passes none, the other factors of that (n, c) still do).
// Backward, coarse to fine, one k_ms_bwd launch per level: k_ssim_bwd's scheme (recompute the coefficients of the 26 x 26
// positions that reach a 16 x 16 pixel tile under one shift per tile, then the transposed passes), scaled per channel by
// gout coef[n][c][j] / positions_j, the coefficients of cs alone for j < K - 1 (sl_point_cs).  The launch of level j also adds
// the pooling adjoint, 1/4 of level j + 1's gradient at (y / 2, x / 2) for y < 2 H_{j+1}, x < 2 W_{j+1}, and writes level j's
// gradient whole: every level is written once and read once, in launch order on one stream.  No float atomics anywhere: the
// same input gives the same bits.
//
// Workspace (vcg_msssim_loss_workspace), kept from the forward to the backward: per level j = 1 .. K - 1 the pooled a, b and
// the gradient map ((N, H_j, W_j, 4) each), then the slots (doubles, [level][n][c][tile]), the factors f (doubles, [n][c][j])
// and coef (floats, [n][c][j]).
#include <math.h>

#include "ssim_window.h"
#include "vcg_common.h"

#define MS_MAX 5
#define MS_FLOOR 1e-4

struct MsP {
  const float4* a;       // this level's generated, (N, H, W, 4)
  const float4* b;       // target
  double* slots;         // this level's [N][3][tiles_y * tiles_x]
  const float* coef;     // [N][3][K]
  const float* gout;     // gout[0], read on the device
  const float4* gc;      // the coarser level's gradient (N, Hc, Wc, 4), null on the last level
  float4* ga;            // this level's gradient (N, H, W, 4)
  float4* pa;            // k_ms_pool: the next level of a and b, (N, H / 2, W / 2, 4)
  float4* pb;
  int H, W, tiles_x, tiles_y, Hc, Wc, level, K, cs;
  float inv_pos;         // 1 / ((H - 10)(W - 10))
  float w[SL_WIN];
};

struct MsFinalP {
  const double* slots;
  double* fac;           // [N][3][K]
  float* coef;           // [N][3][K]
  float* out;
  int N, K;
  int tiles[MS_MAX];
  long long off[MS_MAX]; // first slot of a level
  double inv_pos[MS_MAX], wgt[MS_MAX];
};

__global__ __launch_bounds__(256) void k_ms_pool(MsP p) {
  const int Ho = p.H / 2, Wo = p.W / 2, n = blockIdx.y;
  const size_t in_img = (size_t)blockIdx.x * 256 + threadIdx.x;       // the output pixel within image n
  if (in_img >= (size_t)Ho * Wo) return;
  const int y = (int)(in_img / Wo), x = (int)(in_img - (size_t)y * Wo);
  const size_t i = (size_t)n * Ho * Wo + in_img;
  const size_t src = ((size_t)n * p.H + 2 * y) * p.W + 2 * x;         // rows 2 y + 1 < H and columns 2 x + 1 < W: inside the image
  const float4 a0 = p.a[src], a1 = p.a[src + 1], a2 = p.a[src + p.W], a3 = p.a[src + p.W + 1];
  const float4 b0 = p.b[src], b1 = p.b[src + 1], b2 = p.b[src + p.W], b3 = p.b[src + p.W + 1];
  p.pa[i] = make_float4(0.25f * ((a0.x + a1.x) + (a2.x + a3.x)), 0.25f * ((a0.y + a1.y) + (a2.y + a3.y)),
                        0.25f * ((a0.z + a1.z) + (a2.z + a3.z)), 0.f);
  p.pb[i] = make_float4(0.25f * ((b0.x + b1.x) + (b2.x + b3.x)), 0.25f * ((b0.y + b1.y) + (b2.y + b3.y)),
                        0.25f * ((b0.z + b1.z) + (b2.z + b3.z)), 0.f);
}

__global__ __launch_bounds__(SL_THREADS) void k_ms_fwd(MsP p) {
  __shared__ float sa[3][SL_FS * SL_FS], sb[3][SL_FS * SL_FS];
  __shared__ double vm[5 * SL_FP * SL_FS];
  __shared__ double red[3][SL_THREADS];
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * SL_FP, x0 = blockIdx.x * SL_FP;
  const size_t first = ((size_t)n * p.H + y0) * p.W + x0;           // a valid position: inside the image
  const float4 ka4 = p.a[first], kb4 = p.b[first];
  const float ka[3] = {ka4.x, ka4.y, ka4.z}, kb[3] = {kb4.x, kb4.y, kb4.z};
  sl_stage<SL_FS>(p, n, y0, x0, ka, kb, sa, sb);
  __syncthreads();
  const int r = tid / SL_FP, c = tid - r * SL_FP;
  const bool valid = y0 + r < p.H - SL_HALO && x0 + c < p.W - SL_HALO;
  for (int ch = 0; ch < 3; ++ch) {
    sl_vertical<SL_FP>(p, sa[ch], sb[ch], vm);
    __syncthreads();
    float S = 0.f, A, B, C;
    if (valid) {
      double m[5];
      sl_horizontal<SL_FP>(p, vm, r, c, m);
      if (p.cs) sl_point_cs(m, S, A, B, C);
      else sl_point(m, ka[ch], kb[ch], S, A, B, C);
    }
    red[ch][tid] = (double)S;
    __syncthreads();
  }
  for (int h = SL_THREADS / 2; h > 0; h >>= 1) {   // fixed-order tree, the three channels side by side
    if (tid < h) {
      red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; red[2][tid] += red[2][tid + h];
    }
    __syncthreads();
  }
  if (tid < 3) {
    const size_t tiles = (size_t)p.tiles_y * p.tiles_x;
    p.slots[((size_t)n * 3 + tid) * tiles + (size_t)blockIdx.y * p.tiles_x + blockIdx.x] = red[tid][0];
  }
}

__global__ __launch_bounds__(256) void k_ms_final(MsFinalP p) {
  __shared__ double red[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long sums = (long long)p.N * 3 * p.K;
  for (long long t = wave; t < sums; t += 4) {                       // one wave per (n, c, level): lane-strided, then a fixed butterfly
    const long long nc = t / p.K;
    const int j = (int)(t - nc * p.K);
    const double* s = p.slots + p.off[j] + nc * p.tiles[j];
    double v = 0.0;
    for (int i = lane; i < p.tiles[j]; i += 64) v += s[i];
    v = wave_sum_d(v);
    if (lane == 0) p.fac[t] = v * p.inv_pos[j];
  }
  __syncthreads();                                                     // the factors are read by other waves of this workgroup
  const double inv_nc = 1.0 / (3.0 * (double)p.N);
  double acc = 0.0;
  for (long long nc = tid; nc < (long long)p.N * 3; nc += 256) {
    double ms = 1.0;
    for (int j = 0; j < p.K; ++j) {
      const double f = p.fac[nc * p.K + j];
      ms *= pow(f < MS_FLOOR ? MS_FLOOR : f, p.wgt[j]);
    }
    for (int j = 0; j < p.K; ++j) {
      const double f = p.fac[nc * p.K + j];
      p.coef[nc * p.K + j] = f < MS_FLOOR ? 0.f : (float)(-inv_nc * ms * p.wgt[j] / f);
    }
    acc += ms;
  }
  red[tid] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) p.out[0] = (float)(1.0 - red[0] * inv_nc);
}

__global__ __launch_bounds__(SL_THREADS) void k_ms_bwd(MsP p) {
  __shared__ float sa[SL_BS * SL_BS], sb[SL_BS * SL_BS];              // one channel at a time: the double moments take the room
  __shared__ double vm[5 * SL_BP * SL_BS];                            // the transposed vertical pass reuses it (vt below)
  __shared__ float cf[3][SL_BP * SL_BP];                              // A', B, C of the positions; 0 where a position is not valid
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * SL_TILE, x0 = blockIdx.x * SL_TILE;
  const size_t first = ((size_t)n * p.H + y0) * p.W + x0;           // the tile's first pixel: inside the image
  const float4 ka4 = p.a[first], kb4 = p.b[first];
  const float ka[3] = {ka4.x, ka4.y, ka4.z}, kb[3] = {kb4.x, kb4.y, kb4.z};
  const int py0 = y0 - SL_HALO, px0 = x0 - SL_HALO;                  // first position / first staged pixel
  const float gout = p.gout[0];
  const int r = tid / SL_TILE, c = tid - r * SL_TILE;
  float* vt = (float*)vm;                                             // [3][SL_TILE][SL_BP]
  float g[3];
  for (int ch = 0; ch < 3; ++ch) {
    const float scale = gout * p.coef[((size_t)n * 3 + ch) * p.K + p.level] * p.inv_pos;
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
        if (p.cs) sl_point_cs(m, S, A, B, C);
        else sl_point(m, ka[ch], kb[ch], S, A, B, C);
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
  const int y = y0 + r, x = x0 + c;
  if (y < p.H && x < p.W) {
    if (p.gc && y < 2 * p.Hc && x < 2 * p.Wc) {                      // the pooling adjoint; a dropped odd row or column gets none
      const float4 q = p.gc[((size_t)n * p.Hc + (y >> 1)) * p.Wc + (x >> 1)];
      g[0] += 0.25f * q.x; g[1] += 0.25f * q.y; g[2] += 0.25f * q.z;
    }
    p.ga[((size_t)n * p.H + y) * p.W + x] = make_float4(g[0], g[1], g[2], 0.f);
  }
}

static const double kMsWeights[MS_MAX] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

// the largest K in 1..5 that an H x W image allows (0: not even one window fits)
static int ms_max_scales(int H, int W) {
  const int m = H < W ? H : W;
  int k = 0;
  while (k < MS_MAX && (m >> k) >= SL_WIN) ++k;
  return k;
}

static int ms_args(const char* who, int N, int H, int W, int K) {
  VCG_CHECK_ARG(N > 0 && N <= 65535, "%s: bad N=%d", who, N);
  VCG_CHECK_ARG(K >= 1 && K <= MS_MAX, "%s: scales=%d outside 1..%d", who, K, MS_MAX);
  VCG_CHECK_ARG(H > 0 && W > 0 && H <= 32768 && W <= 32768, "%s: bad H=%d W=%d (1 .. 32768)", who, H, W);
  VCG_CHECK_ARG(ms_max_scales(H, W) >= K,
                "%s: H=%d W=%d too small for scales=%d (the 11x11 window needs min(H, W) >> (scales - 1) >= 11): at most %d scales",
                who, H, W, K, ms_max_scales(H, W));
  return 0;
}

// where everything lives in the workspace; every block is a multiple of 16 bytes
struct MsLayout {
  int H[MS_MAX], W[MS_MAX], tx[MS_MAX], ty[MS_MAX];
  size_t a[MS_MAX], b[MS_MAX], g[MS_MAX];      // byte offsets of level j >= 1
  size_t slot[MS_MAX];                         // first slot (in doubles) of level j
  size_t slots, fac, coef, bytes;              // byte offsets, total
};

static int ms_layout(const char* who, int N, int H, int W, int K, MsLayout* L) {
  if (ms_args(who, N, H, W, K) != 0) return -1;
  size_t at = 0, nslots = 0;
  for (int j = 0; j < K; ++j) {
    L->H[j] = H >> j; L->W[j] = W >> j;
    L->tx[j] = (L->W[j] - SL_HALO + SL_FP - 1) / SL_FP;
    L->ty[j] = (L->H[j] - SL_HALO + SL_FP - 1) / SL_FP;
    L->slot[j] = nslots;
    nslots += (size_t)N * 3 * L->tx[j] * L->ty[j];
    if (j > 0) {
      const size_t level = (size_t)N * L->H[j] * L->W[j] * sizeof(float4);
      L->a[j] = at; L->b[j] = at + level; L->g[j] = at + 2 * level;
      at += 3 * level;
    }
  }
  VCG_CHECK_ARG(nslots <= 0x7FFFFFFFu, "%s: N=%d H=%d W=%d has too many tiles", who, N, H, W);
  const size_t nf = (size_t)N * 3 * K;
  L->slots = at; at += (nslots * sizeof(double) + 15) / 16 * 16;
  L->fac = at;   at += (nf * sizeof(double) + 15) / 16 * 16;
  L->coef = at;  at += (nf * sizeof(float) + 15) / 16 * 16;
  L->bytes = at;
  return 0;
}

static void ms_level(MsP& p, const MsLayout& L, const float* a, const float* b, char* ws, int j, int K) {
  memset(&p, 0, sizeof(p));
  p.a = j == 0 ? (const float4*)a : (const float4*)(ws + L.a[j]);
  p.b = j == 0 ? (const float4*)b : (const float4*)(ws + L.b[j]);
  p.slots = (double*)(ws + L.slots) + L.slot[j];
  p.coef = (const float*)(ws + L.coef);
  p.H = L.H[j]; p.W = L.W[j]; p.tiles_x = L.tx[j]; p.tiles_y = L.ty[j];
  p.level = j; p.K = K; p.cs = j < K - 1;
  p.inv_pos = (float)(1.0 / ((double)(p.H - SL_HALO) * (double)(p.W - SL_HALO)));
  sl_window(p.w);
}

extern "C" size_t vcg_msssim_loss_workspace(int N, int H, int W, int scales) {
  MsLayout L;
  if (ms_layout("vcg_msssim_loss_workspace", N, H, W, scales, &L) != 0) return 0;
  return L.bytes;
}

extern "C" int vcg_msssim_loss_fwd(const float* a, const float* b, float* out, int N, int H, int W, int scales, void* ws,
                                   size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(a && b && out && ws, "vcg_msssim_loss_fwd: null pointer");
  MsLayout L;
  if (ms_layout("vcg_msssim_loss_fwd", N, H, W, scales, &L) != 0) return -1;
  VCG_CHECK_ARG(ws_bytes >= L.bytes, "vcg_msssim_loss_fwd: workspace of %zu bytes, %zu needed", ws_bytes, L.bytes);
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_msssim_loss_fwd: workspace not 16-byte aligned");
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "vcg_msssim_loss_fwd: images not 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  MsFinalP f;
  memset(&f, 0, sizeof(f));
  double wsum = 0.0;
  for (int j = 0; j < scales; ++j) wsum += kMsWeights[j];
  for (int j = 0; j < scales; ++j) {
    MsP p;
    ms_level(p, L, a, b, (char*)ws, j, scales);
    hipLaunchKernelGGL(k_ms_fwd, dim3(p.tiles_x, p.tiles_y, N), dim3(SL_THREADS), 0, st, p);
    if (j + 1 < scales) {
      p.pa = (float4*)((char*)ws + L.a[j + 1]); p.pb = (float4*)((char*)ws + L.b[j + 1]);
      const int per_image = L.H[j + 1] * L.W[j + 1];
      hipLaunchKernelGGL(k_ms_pool, dim3((per_image + 255) / 256, N), dim3(256), 0, st, p);
    }
    f.tiles[j] = p.tiles_x * p.tiles_y;
    f.off[j] = (long long)L.slot[j];
    f.inv_pos[j] = 1.0 / ((double)(p.H - SL_HALO) * (double)(p.W - SL_HALO));
    f.wgt[j] = kMsWeights[j] / wsum;
  }
  f.slots = (const double*)((char*)ws + L.slots); f.fac = (double*)((char*)ws + L.fac); f.coef = (float*)((char*)ws + L.coef);
  f.out = out; f.N = N; f.K = scales;
  hipLaunchKernelGGL(k_ms_final, dim3(1), dim3(256), 0, st, f);
  VCG_LAUNCH_CHECK("vcg_msssim_loss_fwd");
  return 0;
}

extern "C" int vcg_msssim_loss_bwd(const float* a, const float* b, const float* gout, float* ga, int N, int H, int W, int scales,
                                   void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(a && b && gout && ga && ws, "vcg_msssim_loss_bwd: null pointer");
  MsLayout L;
  if (ms_layout("vcg_msssim_loss_bwd", N, H, W, scales, &L) != 0) return -1;
  VCG_CHECK_ARG(ws_bytes >= L.bytes, "vcg_msssim_loss_bwd: workspace of %zu bytes, %zu needed", ws_bytes, L.bytes);
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_msssim_loss_bwd: workspace not 16-byte aligned");
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)ga) & 15) == 0, "vcg_msssim_loss_bwd: images not 16-byte aligned");
  for (int j = scales - 1; j >= 0; --j) {
    MsP p;
    ms_level(p, L, a, b, (char*)ws, j, scales);
    p.gout = gout;
    p.ga = j == 0 ? (float4*)ga : (float4*)((char*)ws + L.g[j]);
    if (j + 1 < scales) {
      p.gc = (const float4*)((char*)ws + L.g[j + 1]);
      p.Hc = L.H[j + 1]; p.Wc = L.W[j + 1];
    }
    hipLaunchKernelGGL(k_ms_bwd, dim3((p.W + SL_TILE - 1) / SL_TILE, (p.H + SL_TILE - 1) / SL_TILE, N), dim3(SL_THREADS), 0,
                       (hipStream_t)stream, p);
  }
  VCG_LAUNCH_CHECK("vcg_msssim_loss_bwd");
  return 0;
}
