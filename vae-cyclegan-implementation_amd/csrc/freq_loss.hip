// Focal frequency loss (Jiang et al., ICCV 2021; patch_factor 1, no ave_spectrum / log_matrix / batch_matrix): the squared
// distance between the orthonormal 2-D spectra of generated and target, every frequency weighted by how badly it is missed,
// forward and the gradient with respect to the generated image.  Operands are (N, H, W, 4) fp32, channel 3 is padding and is
// never read.  H, W in 1 .. VCG_FREQ_MAX_SIDE, independent; alpha >= 0.  With d = a - b, per plane (image n, channel c):
//
//   D = F_H d F_W,   F_n[j, k] = exp(-2 pi i j k / n) / sqrt(n)        p = |D|^2,   m = |D|^alpha (alpha = 0: m = 1)
//   w = m / max over the plane of m (0 where that max is 0), clamped to [0, 1], a constant for the gradient
//   loss = 1 / (3 N H W) sum w p            ga = gout 2 / (3 N H W) Re(F_H^H (w . D) F_W^H),  channel 3 = 0
//
// The package has no FFT and the training sizes are not powers of two, so the DFT is the two matrix products above, one code
// path for every length, on the full-fp32 MFMA (v_mfma_f32_32x32x2_f32).  The twiddle matrices never exist in memory: a table
// of n entries (cos, sin)(2 pi t / n) / sqrt(n) per axis is built once per call with sincospi in double (k_ff_table), every
// workgroup copies the table of the axis it transforms to LDS and fills a twiddle tile by looking up (j k) mod n — integer
// arithmetic, j k < 2^22 — so no trigonometric function ever sees an unreduced argument.  The Hermitian symmetry of a real
// plane's spectrum is not used: the spectrum is stored whole, [plane = 3 n + c][u][v] float2.
//
// k_ff_gemm<MODE>: 256 threads, a 64 x 64 output tile, one 32 x 32 MFMA tile per wavefront, K in chunks of 32 staged in LDS
// with zero fill outside the matrices (H, W and 3 N H that are no tile multiple are the common case).
//   MODE 0  forward rows     R[r][v] = sum_x d[r][x] F_W[x][v]          r = (n H + y) 3 + c over all 3 N H rows; d read from a, b
//   MODE 1  forward columns  D[u][v] = sum_y F_H[u][y] R[y][v]          per plane; also max of p over the tile -> tilemax
//   MODE 2  adjoint columns  T[y][v] = sum_u conj(F_H[u][y]) w D[u][v]  per plane; w . D formed while the tile is staged
//   MODE 3  adjoint rows     ga[r][x] = gout 2 / (3 N H W) Re sum_v T[r][v] conj(F_W[v][x]);  every pixel, channel 3 = 0
// k_ff_finish: per plane and chunk of 4096 frequencies: the plane's maximum from the tile maxima (a maximum is exact, so its
// order does not matter), then sum w p in double -> the chunk's own slot; chunk 0 keeps the plane maximum beside the spectrum
// for the backward.  k_ff_final (one workgroup) adds the slots in a fixed order and applies 1 / (3 N H W).  No float atomics:
// the same input gives the same bits.  A NaN operand makes its plane's spectrum, maximum and sum NaN; only the 0 / 0 of an
// all-zero spectrum maps to weight 0.
#include "vcg_common.h"
#include <math.h>

#define FF_TM 64
#define FF_TN 64
#define FF_TK 32
#define FF_LD 65                  // row pitch of an LDS tile [k][64]: k-fastest staging writes and i-fastest reads both spread over banks
#define FF_THREADS 256
#define FF_CHUNK 4096             // frequencies per k_ff_finish workgroup
#define FF_MAX_N 21845            // 3 N planes on grid.z

struct FreqP {
  const float* a;          // generated, (N, H, W, 4)
  const float* b;          // target
  const float2* tabH;      // H entries (cos, sin)(2 pi t / H) / sqrt(H)
  const float2* tabW;
  const float2* src;       // complex input of MODE 1 .. 3 and of k_ff_finish, [plane][row][col]
  float2* dst;             // complex output of MODE 0 .. 2
  float* tilemax;          // [plane][tiles_plane]: MODE 1 writes, k_ff_finish reads
  float* pmax_out;         // [plane]: k_ff_finish writes (the tail of the kept spectrum)
  const float* pmax;       // [plane]: MODE 2 reads
  double* slots;           // [plane][chunks]
  float* out;              // out[0] = the loss
  const float* gout;       // gout[0], read on the device
  float* ga;               // (N, H, W, 4)
  int N, H, W, P;          // P = 3 N planes
  int tiles_plane, chunks;
  float alpha, gscale;     // gscale = 2 / (3 N H W)
  double inv_count;        // 1 / (3 N H W)
  FastDiv fdH, fdW;
};

// NaN wins
__device__ __forceinline__ float ff_max(float x, float y) { return (x > y || x != x) ? x : y; }
__device__ __forceinline__ float ff_p(float2 d) { return fmaf(d.x, d.x, d.y * d.y); }
// |D|^alpha from p = |D|^2
__device__ __forceinline__ float ff_pow(float p, float alpha) {
  if (alpha == 0.f) return 1.f;
  if (alpha == 1.f) return sqrtf(p);
  return powf(p, 0.5f * alpha);
}
// mmax = ff_pow(plane maximum of p): the same function of the same bits in forward and backward
__device__ __forceinline__ float ff_weight(float p, float mmax, float alpha) {
  if (mmax == 0.f) return 0.f;                             // an all-zero spectrum: 0 / 0 -> 0
  const float w = ff_pow(p, alpha) / mmax;
  return w < 0.f ? 0.f : (w > 1.f ? 1.f : w);              // a NaN stays
}

__global__ __launch_bounds__(256) void k_ff_table(float2* tabH, int H, float2* tabW, int W) {
  int i = blockIdx.x * 256 + threadIdx.x;
  float2* tab = tabH;
  int n = H;
  if (i >= H) { i -= H; tab = tabW; n = W; }
  if (i >= n) return;
  double s, c;
  sincospi((double)(2 * i) / (double)n, &s, &c);           // argument in [0, 2)
  const double r = 1.0 / sqrt((double)n);
  tab[i] = make_float2((float)(c * r), (float)(s * r));
}

// row r of the 3 N H image rows -> first element of that row in a [plane][y][col] complex array, and in the images
struct FfRow { size_t cplx, img; int c; };
__device__ __forceinline__ FfRow ff_row(const FreqP& p, int r) {
  const uint32_t pix = (uint32_t)r / 3u;                   // n H + y
  uint32_t n, y;
  fd_divmod(pix, p.fdH, n, y);
  FfRow o;
  o.c = r - 3 * (int)pix;
  o.cplx = (((size_t)n * 3 + o.c) * p.H + y) * p.W;
  o.img = (size_t)pix * p.W * 4 + o.c;
  return o;
}

template <int MODE>
__global__ __launch_bounds__(FF_THREADS) void k_ff_gemm(FreqP p) {
  constexpr bool ROW = MODE == 0 || MODE == 3;
  constexpr int NT = MODE == 0 ? 3 : 4;
  extern __shared__ float2 s_tab[];                        // the table of the transformed axis
  __shared__ float sT[NT][FF_TK * FF_LD];
  float* sA0 = sT[0];                                      // A[k][i]: MODE 0 d, MODE 3 Re T, MODE 1 / 2 cos
  float* sB0 = sT[1];                                      // B[k][j]: ROW cos, MODE 1 / 2 Re X
  float* sB1 = sT[2];                                      //          ROW -sin, MODE 1 / 2 Im X
  float* sA1 = sT[NT - 1];                                 // MODE 3 Im T, MODE 1 sin, MODE 2 -sin (MODE 0: unused)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int K = ROW ? p.W : p.H;                           // the transformed length
  const int M = ROW ? 3 * p.N * p.H : p.H;
  const int NC = p.W;
  const FastDiv fd = ROW ? p.fdW : p.fdH;
  const float2* tab = ROW ? p.tabW : p.tabH;
  const int m0 = (ROW ? blockIdx.x : blockIdx.y) * FF_TM, n0 = (ROW ? blockIdx.y : blockIdx.x) * FF_TN;
  const int z = ROW ? 0 : blockIdx.z;
  for (int i = tid; i < K; i += FF_THREADS) s_tab[i] = tab[i];
  float mmax = 0.f;
  if (MODE == 2) mmax = ff_pow(p.pmax[z], p.alpha);
  const float2* X = ROW ? p.src : p.src + (size_t)z * p.H * p.W;

  f32x16 acc0, acc1;
#pragma unroll
  for (int q = 0; q < 16; ++q) { acc0[q] = 0.f; acc1[q] = 0.f; }

  for (int k0 = 0; k0 < K; k0 += FF_TK) {
    __syncthreads();                                       // the last chunk's reads are done (first pass: s_tab is written)
    // ---- A tile
    if (ROW) {
      for (int e = tid; e < FF_TM * FF_TK; e += FF_THREADS) {          // k fastest: along the rows in memory
        const int kk = e & (FF_TK - 1), i = e >> 5, r = m0 + i, k = k0 + kk;
        float v0 = 0.f, v1 = 0.f;
        if (r < M && k < K) {
          const FfRow row = ff_row(p, r);
          if (MODE == 0) {
            const size_t at = row.img + (size_t)k * 4;
            v0 = p.a[at] - p.b[at];
          } else {
            const float2 t = X[row.cplx + k];
            v0 = t.x; v1 = t.y;
          }
        }
        sA0[kk * FF_LD + i] = v0;
        if (MODE == 3) sA1[kk * FF_LD + i] = v1;
      }
    } else {
      for (int e = tid; e < FF_TM * FF_TK; e += FF_THREADS) {
        const int i = e & (FF_TM - 1), kk = e >> 6, u = m0 + i, y = k0 + kk;
        float2 t = make_float2(0.f, 0.f);
        if (u < M && y < K) {
          uint32_t q, rem;
          fd_divmod((uint32_t)u * (uint32_t)y, fd, q, rem);
          t = s_tab[rem];
        }
        sA0[kk * FF_LD + i] = t.x;
        sA1[kk * FF_LD + i] = MODE == 1 ? t.y : -t.y;
      }
    }
    // ---- B tile
    for (int e = tid; e < FF_TN * FF_TK; e += FF_THREADS) {
      const int j = e & (FF_TN - 1), kk = e >> 6, col = n0 + j, k = k0 + kk;
      float2 t = make_float2(0.f, 0.f);
      if (col < NC && k < K) {
        if (ROW) {
          uint32_t q, rem;
          fd_divmod((uint32_t)k * (uint32_t)col, fd, q, rem);
          t = s_tab[rem];
          t.y = -t.y;
        } else {
          t = X[(size_t)k * p.W + col];
          if (MODE == 2) {
            const float w = ff_weight(ff_p(t), mmax, p.alpha);
            t.x *= w; t.y *= w;
          }
        }
      }
      sB0[kk * FF_LD + j] = t.x;
      sB1[kk * FF_LD + j] = t.y;
    }
    __syncthreads();
    // ---- lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31] of a 32 x 32 x 2 step
#pragma unroll 4
    for (int kk = 0; kk < FF_TK; kk += 2) {
      const int k = kk + (lane >> 5);
      const int ia = k * FF_LD + wm * 32 + (lane & 31), ib = k * FF_LD + wn * 32 + (lane & 31);
      if (MODE == 0) {
        const float x = sA0[ia];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, sB0[ib], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, sB1[ib], acc1, 0, 0, 0);
      } else if (MODE == 3) {                              // Re((Tre + i Tim)(c + i s)) = Tre c + Tim (-s)
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sA0[ia], sB0[ib], acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sA1[ia], sB1[ib], acc0, 0, 0, 0);
      } else {                                             // (c - i t)(Xre + i Xim), t = +sin (MODE 1) or -sin (MODE 2)
        const float c = sA0[ia], t = sA1[ia], xr = sB0[ib], xi = sB1[ib];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(c, xr, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(t, xi, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c, xi, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(-t, xr, acc1, 0, 0, 0);
      }
    }
  }

  // ---- C: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = n0 + wn * 32 + (lane & 31);
  const float go = MODE == 3 ? p.gout[0] * p.gscale : 0.f;
  float pm = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = m0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
    if (row >= M || col >= NC) continue;
    if (MODE == 0) {
      p.dst[ff_row(p, row).cplx + col] = make_float2(acc0[q], acc1[q]);
    } else if (MODE == 3) {
      const FfRow r = ff_row(p, row);
      float* g = p.ga + r.img + (size_t)col * 4;
      g[0] = go * acc0[q];
      if (r.c == 0) g[3] = 0.f;
    } else {
      const float2 d = make_float2(acc0[q], acc1[q]);
      p.dst[((size_t)z * p.H + row) * p.W + col] = d;
      if (MODE == 1) pm = ff_max(pm, ff_p(d));
    }
  }
  if (MODE == 1) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pm = ff_max(pm, __shfl_xor(pm, o, 64));
    __syncthreads();                                       // the tiles are free
    if (lane == 0) sA0[wave] = pm;
    __syncthreads();
    if (tid == 0)
      p.tilemax[(size_t)z * p.tiles_plane + blockIdx.y * gridDim.x + blockIdx.x] =
          ff_max(ff_max(sA0[0], sA0[1]), ff_max(sA0[2], sA0[3]));
  }
}

__global__ __launch_bounds__(256) void k_ff_finish(FreqP p) {
  __shared__ float smax[256 / VCG_WAVE];
  __shared__ double sred[256 / VCG_WAVE];
  const int tid = threadIdx.x, z = blockIdx.y, chunk = blockIdx.x;
  float pm = 0.f;
  for (int i = tid; i < p.tiles_plane; i += 256) pm = ff_max(pm, p.tilemax[(size_t)z * p.tiles_plane + i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pm = ff_max(pm, __shfl_xor(pm, o, 64));
  if ((tid & (VCG_WAVE - 1)) == 0) smax[tid / VCG_WAVE] = pm;
  __syncthreads();
  pm = ff_max(ff_max(smax[0], smax[1]), ff_max(smax[2], smax[3]));
  if (chunk == 0 && tid == 0) p.pmax_out[z] = pm;
  const float mmax = ff_pow(pm, p.alpha);
  const int HW = p.H * p.W;
  const float2* D = p.src + (size_t)z * HW;
  const int end = min(HW, (chunk + 1) * FF_CHUNK);
  double acc = 0.0;
  for (int i = chunk * FF_CHUNK + tid; i < end; i += 256) {
    const float pw = ff_p(D[i]);
    acc += (double)ff_weight(pw, mmax, p.alpha) * (double)pw;
  }
  acc = wave_sum_d(acc);
  if ((tid & (VCG_WAVE - 1)) == 0) sred[tid / VCG_WAVE] = acc;
  __syncthreads();
  if (tid == 0) p.slots[(size_t)z * p.chunks + chunk] = ((sred[0] + sred[1]) + sred[2]) + sred[3];
}

__global__ __launch_bounds__(256) void k_ff_final(FreqP p) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const size_t total = (size_t)p.P * p.chunks;
  double s = 0.0;
  for (size_t i = tid; i < total; i += 256) s += p.slots[i];
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) p.out[0] = (float)(red[0] * p.inv_count);
}

// ---- host ------------------------------------------------------------------------------------------------------------------

static size_t ff_pad16(size_t bytes) { return (bytes + 15) / 16 * 16; }

static int ff_args(const char* who, int N, int H, int W) {
  VCG_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: bad N=%d H=%d W=%d", who, N, H, W);
  VCG_CHECK_ARG(H <= VCG_FREQ_MAX_SIDE && W <= VCG_FREQ_MAX_SIDE, "%s: H=%d W=%d above the side cap %d", who, H, W,
                VCG_FREQ_MAX_SIDE);
  VCG_CHECK_ARG(N <= FF_MAX_N, "%s: N=%d above %d", who, N, FF_MAX_N);
  return 0;
}

static int ff_alpha(const char* who, float alpha) {
  VCG_CHECK_ARG(alpha >= 0.f && alpha <= 3.0e38f, "%s: alpha=%g must be finite and >= 0", who, (double)alpha);
  return 0;
}

struct FfLayout {                  // byte offsets into the workspace and the kept state
  size_t tabH, tabW, cplx, tilemax, slots, ws_bytes;       // workspace: tables, R (forward) or T (backward), maxima, slots
  size_t pmax, spec_bytes;                                 // kept state: D at 0, plane maxima at pmax
  int tiles_x, tiles_y, chunks;
};

static FfLayout ff_layout(int N, int H, int W) {
  FfLayout L;
  const size_t P = (size_t)3 * N, HW = (size_t)H * W;
  L.tiles_x = (W + FF_TN - 1) / FF_TN;
  L.tiles_y = (H + FF_TM - 1) / FF_TM;
  L.chunks = (int)((HW + FF_CHUNK - 1) / FF_CHUNK);
  L.tabH = 0;
  L.tabW = L.tabH + ff_pad16((size_t)H * sizeof(float2));
  L.cplx = L.tabW + ff_pad16((size_t)W * sizeof(float2));
  L.tilemax = L.cplx + ff_pad16(P * HW * sizeof(float2));
  L.slots = L.tilemax + ff_pad16(P * L.tiles_x * L.tiles_y * sizeof(float));
  L.ws_bytes = L.slots + ff_pad16(P * L.chunks * sizeof(double));
  L.pmax = ff_pad16(P * HW * sizeof(float2));
  L.spec_bytes = L.pmax + ff_pad16(P * sizeof(float));
  return L;
}

extern "C" size_t vcg_freq_loss_workspace(int N, int H, int W) {
  if (ff_args("vcg_freq_loss_workspace", N, H, W) != 0) return 0;
  return ff_layout(N, H, W).ws_bytes;
}

extern "C" size_t vcg_freq_loss_spectrum(int N, int H, int W) {
  if (ff_args("vcg_freq_loss_spectrum", N, H, W) != 0) return 0;
  return ff_layout(N, H, W).spec_bytes;
}

static void ff_fill(FreqP& p, const FfLayout& L, int N, int H, int W, float alpha, void* ws) {
  memset(&p, 0, sizeof(p));
  char* w = (char*)ws;
  p.tabH = (const float2*)(w + L.tabH);
  p.tabW = (const float2*)(w + L.tabW);
  p.tilemax = (float*)(w + L.tilemax);
  p.slots = (double*)(w + L.slots);
  p.N = N; p.H = H; p.W = W; p.P = 3 * N;
  p.tiles_plane = L.tiles_x * L.tiles_y;
  p.chunks = L.chunks;
  p.alpha = alpha;
  p.inv_count = 1.0 / (3.0 * N * H * W);
  p.gscale = (float)(2.0 * p.inv_count);
  p.fdH = make_fastdiv((uint32_t)H);
  p.fdW = make_fastdiv((uint32_t)W);
}

template <int MODE>
static void ff_launch(const FreqP& p, const FfLayout& L, hipStream_t st) {
  constexpr bool ROW = MODE == 0 || MODE == 3;
  const int rows = 3 * p.N * p.H;
  const dim3 grid = ROW ? dim3((rows + FF_TM - 1) / FF_TM, L.tiles_x, 1) : dim3(L.tiles_x, L.tiles_y, p.P);
  const size_t tab_bytes = (size_t)(ROW ? p.W : p.H) * sizeof(float2);
  hipLaunchKernelGGL(k_ff_gemm<MODE>, grid, dim3(FF_THREADS), tab_bytes, st, p);
}

extern "C" int vcg_freq_loss_fwd(const float* a, const float* b, float* out, int N, int H, int W, float alpha, void* spec,
                                 size_t spec_bytes, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(a && b && out && spec && ws, "vcg_freq_loss_fwd: null pointer");
  if (ff_args("vcg_freq_loss_fwd", N, H, W) != 0 || ff_alpha("vcg_freq_loss_fwd", alpha) != 0) return -1;
  const FfLayout L = ff_layout(N, H, W);
  VCG_CHECK_ARG(spec_bytes >= L.spec_bytes, "vcg_freq_loss_fwd: spectrum of %zu bytes, %zu needed", spec_bytes, L.spec_bytes);
  VCG_CHECK_ARG(ws_bytes >= L.ws_bytes, "vcg_freq_loss_fwd: workspace of %zu bytes, %zu needed", ws_bytes, L.ws_bytes);
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)spec | (uintptr_t)ws) & 15) == 0,
                "vcg_freq_loss_fwd: images, spectrum or workspace not 16-byte aligned");
  VCG_CHECK_ARG(((uintptr_t)out & 3) == 0, "vcg_freq_loss_fwd: out not 4-byte aligned");
  FreqP p;
  ff_fill(p, L, N, H, W, alpha, ws);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ff_table, dim3((H + W + 255) / 256), dim3(256), 0, st, (float2*)((char*)ws + L.tabH), H,
                     (float2*)((char*)ws + L.tabW), W);
  p.a = a; p.b = b;
  p.dst = (float2*)((char*)ws + L.cplx);
  ff_launch<0>(p, L, st);
  p.src = (const float2*)((char*)ws + L.cplx);
  p.dst = (float2*)spec;
  ff_launch<1>(p, L, st);
  p.src = (const float2*)spec;
  p.pmax_out = (float*)((char*)spec + L.pmax);
  p.out = out;
  hipLaunchKernelGGL(k_ff_finish, dim3(L.chunks, p.P), dim3(256), 0, st, p);
  hipLaunchKernelGGL(k_ff_final, dim3(1), dim3(256), 0, st, p);
  VCG_LAUNCH_CHECK("vcg_freq_loss_fwd");
  return 0;
}

extern "C" int vcg_freq_loss_bwd(const void* spec, size_t spec_bytes, const float* gout, float* ga, int N, int H, int W,
                                 float alpha, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(spec && gout && ga && ws, "vcg_freq_loss_bwd: null pointer");
  if (ff_args("vcg_freq_loss_bwd", N, H, W) != 0 || ff_alpha("vcg_freq_loss_bwd", alpha) != 0) return -1;
  const FfLayout L = ff_layout(N, H, W);
  VCG_CHECK_ARG(spec_bytes >= L.spec_bytes, "vcg_freq_loss_bwd: spectrum of %zu bytes, %zu needed", spec_bytes, L.spec_bytes);
  VCG_CHECK_ARG(ws_bytes >= L.ws_bytes, "vcg_freq_loss_bwd: workspace of %zu bytes, %zu needed", ws_bytes, L.ws_bytes);
  VCG_CHECK_ARG((((uintptr_t)ga | (uintptr_t)spec | (uintptr_t)ws) & 15) == 0,
                "vcg_freq_loss_bwd: gradient, spectrum or workspace not 16-byte aligned");
  VCG_CHECK_ARG(((uintptr_t)gout & 3) == 0, "vcg_freq_loss_bwd: gout not 4-byte aligned");
  FreqP p;
  ff_fill(p, L, N, H, W, alpha, ws);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ff_table, dim3((H + W + 255) / 256), dim3(256), 0, st, (float2*)((char*)ws + L.tabH), H,
                     (float2*)((char*)ws + L.tabW), W);
  p.src = (const float2*)spec;
  p.pmax = (const float*)((const char*)spec + L.pmax);
  p.dst = (float2*)((char*)ws + L.cplx);
  ff_launch<2>(p, L, st);
  p.src = (const float2*)((char*)ws + L.cplx);
  p.gout = gout; p.ga = ga;
  ff_launch<3>(p, L, st);
  VCG_LAUNCH_CHECK("vcg_freq_loss_bwd");
  return 0;
}
