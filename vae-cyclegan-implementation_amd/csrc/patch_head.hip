// The discriminator head as a sliding (patch) convolution: spectral_norm(nn.Conv2d(512, 1, 16, stride 1, padding 0)) on a map
// larger than its kernel, followed by .view(-1, 1).squeeze(1) (reference Networks.py:248, :269).  One output channel, valid,
// stride 1:  x (N, H, W, C) NHWC, wsn_k[(ky KW + kx) C + c] as vcg_sn_prepare writes it, OH = H - KH + 1, OW = W - KW + 1.
//
//   out[n, oy, ox] = bias + sum_{ky,kx,c} x[n, oy+ky, ox+kx, c] wsn_k[ky, kx, c]
//   dx[n, y, x, c] = sum_{oy,ox} g[n, oy, ox] wsn_k[y-oy, x-ox, c]
//   gk[ky, kx, c]  = sum_{n,oy,ox} g[n, oy, ox] x[n, oy+ky, ox+kx, c]
//
// At 512 x 512 and batch 8 the map is 16 MB, the weight 512 KB and each direction 0.6 GFLOP: the work is moving the map, so
// every direction is organised by INPUT ROW (forward, weight gradient) or OUTPUT ROW (data gradient) of the map, which a
// workgroup touches once, and the taps of the other axis become the K or M dimension of a small GEMM on the full-fp32 MFMA
// (v_mfma_f32_16x16x4_f32: fp32 products, fp32 accumulation, no operand split — the head feeds the LSGAN loss directly).
//
//   forward   per (channel chunk, input row r, 48 flattened (n, ox) rows):  P[(n, ox)][ky] = sum_{kx, c in chunk} x[n, r, ox+kx, c]
//             w[ky, kx, c] — M = (n, ox), N = ky, K = (kx, c); the A operand is a sliding window over the row staged in LDS, so the
//             taps are address offsets.  The four waves split kx and add their tiles through LDS in wave order.  A second kernel
//             adds out[n, oy, ox] = bias + sum_ky sum_chunk P[chunk][n][oy+ky][ox][ky].
//   dgrad     per (256 channels, output row y, 64 flattened (n, x) rows):  dx[(n, x)][c] = sum_{ky valid} sum_kx g[n, y-ky, x-kx]
//             w[ky, kx, c] — M = (n, x), N = c, K = (ky, kx); the g rows, zero-padded by KW - 1 on both sides, sit in LDS.
//             Every element of dx is stored once, none accumulated.
//   wgrad     per (4 ky, 256 channels, input row y):  part[y][ky, kx, c] = sum_n sum_xx g[n, y-ky, xx-kx] x[n, y, xx, c] —
//             M = kx, N = c, K = (n, xx); a second kernel adds the rows that reach each ky in ascending y, takes the dot with
//             wsn_k and the sum of g, and misc.hip's spectral-norm stage (k_fullmap_wgrad2, shared, not restated) finishes.
//
// The K index of an MFMA is a free permutation, and so is the column index: a lane reads FOUR consecutive channels with one
// 16-byte load and feeds them to four MFMAs (as four k in the forward, as four column sets in the gradients), so global and LDS
// reads are float4 and the gradients' stores are float4 too.
//
// Determinism: no atomics; every sum runs in an order fixed by the shapes (k steps ascending, waves 0..3, chunks ascending, a
// fixed xor tree over ky), and an output element of image n is a dot product over image n alone with the same order for every n
// and every batch size (the forward's chunk width is chosen without looking at N) — shards of a batch give the bits of the whole batch.
#include "vcg_common.h"

#define PH_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

namespace {

constexpr int kPhFwdTiles = 3;    // 48 (n, ox) rows per forward workgroup: 8 x 17 = 136 rows fill 3 workgroups to 94 %
constexpr int kPhDgTiles = 4;     // 64 (n, x) rows per data-gradient workgroup
constexpr int kPhLds = 64 * 1024;
constexpr int kPhRedBlocks = 256;

__device__ __forceinline__ float ph_block_sum(float v, float* red4) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  const float tot = ((red4[0] + red4[1]) + red4[2]) + red4[3];
  __syncthreads();
  return tot;
}

// ------------------------------------------------------------------------------------------------------------------ forward
// grid (channel chunks x tiles of 16 kernel rows, H, row groups), 256 threads, LDS max(images x W x (CC + 4), 4 x tiles x 256) floats
template <int CC>
__global__ __launch_bounds__(256) void k_ph_fwd(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ P,
                                                int N, int H, int W, int C, int KH, int KW, int OW, int chunks) {
  extern __shared__ float4 ph_smem4[];
  float* xs = reinterpret_cast<float*>(ph_smem4);
  constexpr int CCP = CC + 4, TM = kPhFwdTiles;
  const int chunk = blockIdx.x % chunks, ky0 = (blockIdx.x / chunks) * 16, KHp = (KH + 15) / 16 * 16;
  const int r = blockIdx.y, m0 = blockIdx.z * 16 * TM, c0 = chunk * CC;
  const int Mtot = N * OW;
  const int mlast = (m0 + 16 * TM < Mtot ? m0 + 16 * TM : Mtot) - 1;
  const int n0 = m0 / OW, nimg = mlast / OW - n0 + 1, ntiles = (mlast - m0) / 16 + 1;
  const int per_img = W * (CC / 4);
  for (int i = threadIdx.x; i < nimg * per_img; i += 256) {
    const int s = i / per_img, rem = i - s * per_img, px = rem / (CC / 4), c4 = rem - px * (CC / 4);
    const int c = c0 + 4 * c4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) v = *reinterpret_cast<const float4*>(x + (((size_t)(n0 + s) * H + r) * W + px) * C + c);
    *reinterpret_cast<float4*>(xs + (s * W + px) * CCP + 4 * c4) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
  int abase[TM];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    int m = m0 + 16 * t + row;
    m = m < mlast ? m : mlast;
    const int n = m / OW, ox = m - n * OW;
    abase[t] = ((n - n0) * W + ox) * CCP + 4 * q;
  }
  f32x4 acc[TM];
#pragma unroll
  for (int t = 0; t < TM; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kx = wave; kx < KW; kx += 4) {
#pragma unroll
    for (int s = 0; s < CC / 16; ++s) {
      const int c = c0 + 16 * s + 4 * q;
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ky0 + row < KH && c < C) b = *reinterpret_cast<const float4*>(w + ((size_t)(ky0 + row) * KW + kx) * C + c);
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        if (t < ntiles) {
          const float4 a = *reinterpret_cast<const float4*>(xs + abase[t] + kx * CCP + 16 * s);
          acc[t] = PH_MFMA(a.x, b.x, acc[t]);
          acc[t] = PH_MFMA(a.y, b.y, acc[t]);
          acc[t] = PH_MFMA(a.z, b.z, acc[t]);
          acc[t] = PH_MFMA(a.w, b.w, acc[t]);
        }
      }
    }
  }
  __syncthreads();                                      // the row slab is dead: its LDS takes the four waves' tiles
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) xs[((wave * TM + t) * 16 + 4 * q + v) * 16 + row] = acc[t][v];
  __syncthreads();
  for (int e = threadIdx.x; e < ntiles * 256; e += 256) {
    const int t = e >> 8, rowd = (e >> 4) & 15, ky = e & 15, m = m0 + 16 * t + rowd;
    if (m > mlast || ky0 + ky >= KH) continue;
    const int in = e & 255;
    const float s = ((xs[(0 * TM + t) * 256 + in] + xs[(1 * TM + t) * 256 + in]) + xs[(2 * TM + t) * 256 + in]) +
                    xs[(3 * TM + t) * 256 + in];
    const int n = m / OW, ox = m - n * OW;
    P[((((size_t)chunk * N + n) * H + r) * OW + ox) * KHp + ky0 + ky] = s;
  }
}

// out[n, oy, ox] = bias + sum_ky sum_chunk P[chunk][n][oy+ky][ox][ky]: 16 lanes per logit, lane l adds ky = l, l + 16, .. with the
// chunks ascending inside, then an xor tree over the lanes
__global__ __launch_bounds__(256) void k_ph_fwd_sum(const float* __restrict__ P, const float* __restrict__ bias,
                                                    float* __restrict__ out, int N, int H, int OH, int OW, int KH, int chunks) {
  const int ky = threadIdx.x & 15;
  const size_t total = (size_t)N * OH * OW;
  const size_t o = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const size_t oc = o < total ? o : total - 1;
  const int ox = (int)(oc % OW), oy = (int)((oc / OW) % OH), n = (int)(oc / ((size_t)OW * OH));
  const int KHp = (KH + 15) / 16 * 16;
  float s = 0.f;
  for (int kk = ky; kk < KH; kk += 16)
    for (int ch = 0; ch < chunks; ++ch) s += P[((((size_t)ch * N + n) * H + oy + kk) * OW + ox) * KHp + kk];
#pragma unroll
  for (int d = 8; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if (ky == 0 && o < total) out[o] = s + (bias ? bias[0] : 0.f);
}

// ------------------------------------------------------------------------------------------------------------ data gradient
// grid (ceil(C / 256), H, row groups), 256 threads: wave w owns channels 64 w .. 64 w + 63 of the block's 256
__global__ __launch_bounds__(256) void k_ph_dgrad(const float* __restrict__ g, const float* __restrict__ w, float* __restrict__ dx,
                                                  int N, int H, int W, int C, int KH, int KW, int OH, int OW) {
  extern __shared__ float4 ph_smem4[];
  float* gs = reinterpret_cast<float*>(ph_smem4);
  constexpr int TM = kPhDgTiles;
  const int y = blockIdx.y, m0 = blockIdx.z * 16 * TM;
  const int Mtot = N * W;
  const int mlast = (m0 + 16 * TM < Mtot ? m0 + 16 * TM : Mtot) - 1;
  const int n0 = m0 / W, nimg = mlast / W - n0 + 1, ntiles = (mlast - m0) / 16 + 1;
  const int GW = OW + 2 * (KW - 1), per_img = KH * GW;
  for (int i = threadIdx.x; i < nimg * per_img; i += 256) {
    const int s = i / per_img, rem = i - s * per_img, ky = rem / GW, col = rem - ky * GW;
    const int oy = y - ky, ox = col - (KW - 1);
    float v = 0.f;
    if (oy >= 0 && oy < OH && ox >= 0 && ox < OW) v = g[((size_t)(n0 + s) * OH + oy) * OW + ox];
    gs[i] = v;
  }
  __syncthreads();                                      // the only barrier: a wave past the last channel may leave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
  const int c0w = blockIdx.x * 256 + wave * 64;
  if (c0w >= C) return;
  const int cj = c0w + 4 * row;
  const bool cok = cj < C;
  const int kylo = y - OH + 1 > 0 ? y - OH + 1 : 0, kyhi = y < KH - 1 ? y : KH - 1;
  int abase[TM];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    int m = m0 + 16 * t + row;
    m = m < mlast ? m : mlast;
    const int n = m / W, xx = m - n * W;
    abase[t] = (n - n0) * per_img + xx + KW - 1;
  }
  f32x4 acc[TM][4];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ky = kylo; ky <= kyhi; ++ky) {
    for (int k4 = 0; k4 < KW; k4 += 4) {
      const int kx = k4 + q;
      const bool kok = kx < KW;
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kok && cok) b = *reinterpret_cast<const float4*>(w + ((size_t)ky * KW + kx) * C + cj);
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        if (t < ntiles) {
          const float a = kok ? gs[abase[t] + ky * GW - kx] : 0.f;
          acc[t][0] = PH_MFMA(a, b.x, acc[t][0]);
          acc[t][1] = PH_MFMA(a, b.y, acc[t][1]);
          acc[t][2] = PH_MFMA(a, b.z, acc[t][2]);
          acc[t][3] = PH_MFMA(a, b.w, acc[t][3]);
        }
      }
    }
  }
  if (!cok) return;
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    if (t < ntiles) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int m = m0 + 16 * t + 4 * q + v;
        if (m <= mlast) {
          const int n = m / W, xx = m - n * W;
          *reinterpret_cast<float4*>(dx + (((size_t)n * H + y) * W + xx) * C + cj) =
              make_float4(acc[t][0][v], acc[t][1][v], acc[t][2][v], acc[t][3][v]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- weight gradient
// grid (ceil(KH / 4) x tiles of 16 kernel columns, ceil(C / 256), H), 256 threads, no LDS: part[y][(ky KW + kx) C + c] for the (y, ky) pairs with a logit row
__global__ __launch_bounds__(256) void k_ph_wgrad(const float* __restrict__ g, const float* __restrict__ x,
                                                  float* __restrict__ part, int N, int H, int W, int C, int KH, int KW, int OH,
                                                  int OW, int kygroups) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
  const int y = blockIdx.z, c0w = blockIdx.y * 256 + wave * 64;
  const int kyg = blockIdx.x % kygroups, kx0 = (blockIdx.x / kygroups) * 16;
  if (c0w >= C) return;
  const int cj = c0w + 4 * row;
  const bool cok = cj < C;
  int oy[4];
  bool tv[4];
  bool any = false;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ky = kyg * 4 + t;
    oy[t] = y - ky;
    tv[t] = ky < KH && oy[t] >= 0 && oy[t] < OH;
    any = any || tv[t];
  }
  if (!any) return;
  f32x4 acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < N; ++n) {
    const float* xr = x + ((size_t)n * H + y) * W * C;
    for (int x4 = 0; x4 < W; x4 += 4) {
      const int xx = x4 + q;                             // the MFMA's k: an input pixel of this row
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (xx < W && cok) b = *reinterpret_cast<const float4*>(xr + (size_t)xx * C + cj);
      const int ox = xx - kx0 - row;                     // the MFMA's row: kx = kx0 + row
      const bool aok = xx < W && kx0 + row < KW && ox >= 0 && ox < OW;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (tv[t]) {
          const float a = aok ? g[((size_t)n * OH + oy[t]) * OW + ox] : 0.f;
          acc[t][0] = PH_MFMA(a, b.x, acc[t][0]);
          acc[t][1] = PH_MFMA(a, b.y, acc[t][1]);
          acc[t][2] = PH_MFMA(a, b.z, acc[t][2]);
          acc[t][3] = PH_MFMA(a, b.w, acc[t][3]);
        }
      }
    }
  }
  if (!cok) return;
  const size_t K = (size_t)KH * KW * C;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (tv[t]) {
      const int ky = kyg * 4 + t;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int kx = kx0 + 4 * q + v;
        if (kx < KW)
          *reinterpret_cast<float4*>(part + (size_t)y * K + ((size_t)ky * KW + kx) * C + cj) =
              make_float4(acc[t][0][v], acc[t][1][v], acc[t][2][v], acc[t][3][v]);
      }
    }
  }
}

// gk[k] = sum_{oy ascending} part[ky + oy][k]; pdot[block] = sum_k gk[k] wsn_k[k]; gsum[0] = sum of all logit gradients
__global__ __launch_bounds__(256) void k_ph_wgrad_sum(const float* __restrict__ part, const float* __restrict__ w,
                                                      const float* __restrict__ g, float* __restrict__ gk,
                                                      float* __restrict__ pdot, float* __restrict__ gsum, size_t K, size_t KWC,
                                                      int OH, size_t G) {
  __shared__ float red[4];
  float s = 0.f;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < K; k += (size_t)gridDim.x * 256) {
    const size_t ky = k / KWC;
    float acc = 0.f;
    for (int o = 0; o < OH; ++o) acc += part[(ky + o) * K + k];
    gk[k] = acc;
    s += acc * w[k];
  }
  const float tot = ph_block_sum(s, red);
  if (threadIdx.x == 0) pdot[blockIdx.x] = tot;
  if (blockIdx.x == 0) {
    float t = 0.f;
    for (size_t i = threadIdx.x; i < G; i += 256) t += g[i];
    const float gt = ph_block_sum(t, red);
    if (threadIdx.x == 0) gsum[0] = gt;
  }
}

struct PhDims {
  int N, H, W, C, KH, KW, OH, OW;
};

bool ph_dims_ok(int N, int H, int W, int C, int KH, int KW) {
  return N > 0 && C > 0 && C % 4 == 0 && KH > 0 && KW > 0 && H >= KH && W >= KW && (double)N * H * W * C < 2147483648.0 * 4.0 &&
         (double)KH * KW * C * H < 2147483648.0;
}

// images a run of `rows` flattened (image, column) rows can touch when an image has `per` of them
int ph_images(int rows, int per, int N) {
  const int m = (rows - 2) / per + 2;
  return m < N ? m : N;
}

// the forward's channels per workgroup: the widest of 64 / 32 / 16 whose row slab fits the LDS (0: the map is too wide).  The
// chunk count sets the order in which k_ph_fwd_sum adds, so it must not depend on the batch: the slab is sized for the images
// a workgroup could touch in a batch of any size, not for those of this one
int ph_fwd_cc(int W, int C, int OW) {
  const int imgs = ph_images(16 * kPhFwdTiles, OW, 1 << 30);
  for (int cc = 64; cc >= 16; cc /= 2) {
    if (cc > 16 && cc / 2 >= C) continue;
    if ((size_t)imgs * W * (cc + 4) * sizeof(float) <= (size_t)kPhLds) return cc;
  }
  return 0;
}

size_t ph_fwd_lds(int N, int W, int OW, int cc) {
  const size_t slab = (size_t)ph_images(16 * kPhFwdTiles, OW, N) * W * (cc + 4), red = 4 * kPhFwdTiles * 256;
  return (slab > red ? slab : red) * sizeof(float);
}

size_t ph_dgrad_lds(int N, int W, int KH, int KW, int OW) {
  return (size_t)ph_images(16 * kPhDgTiles, W, N) * KH * (OW + 2 * (KW - 1)) * sizeof(float);
}

size_t ph_fwd_ws(int N, int H, int W, int C, int KH, int KW) {
  const int OW = W - KW + 1, cc = ph_fwd_cc(W, C, OW);
  if (!cc) return 0;
  return (size_t)((C + cc - 1) / cc) * N * H * OW * ((KH + 15) / 16 * 16) * sizeof(float);
}

size_t ph_wgrad_ws(int H, int C, int KH, int KW) {
  const size_t K = (size_t)KH * KW * C;
  return ((size_t)H * K + K + kPhRedBlocks + 4) * sizeof(float);
}

}  // namespace

extern "C" size_t vcg_patch_head_workspace(int N, int H, int W, int C, int KH, int KW) {
  if (!ph_dims_ok(N, H, W, C, KH, KW)) {
    vcg_set_error("vcg_patch_head_workspace: bad dims N %d map %dx%dx%d kernel %dx%d (C %% 4 == 0, kernel <= map)", N, C, H, W,
                  KH, KW);
    return 0;
  }
  const size_t f = ph_fwd_ws(N, H, W, C, KH, KW), g = ph_wgrad_ws(H, C, KH, KW);
  if (!f || ph_dgrad_lds(N, W, KH, KW, W - KW + 1) > (size_t)kPhLds) {
    vcg_set_error("vcg_patch_head_workspace: a map row of %d pixels does not fit the on-chip staging", W);
    return 0;
  }
  return ((f > g ? f : g) + 15) / 16 * 16;
}

extern "C" int vcg_patch_head_fwd(const float* x, const float* wsn_k, const float* bias, float* out, int N, int H, int W, int C,
                                  int KH, int KW, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(x && wsn_k && out && ws, "vcg_patch_head_fwd: null pointer");
  VCG_CHECK_ARG(ph_dims_ok(N, H, W, C, KH, KW), "vcg_patch_head_fwd: bad dims N %d map %dx%dx%d kernel %dx%d", N, C, H, W, KH, KW);
  const int OH = H - KH + 1, OW = W - KW + 1, cc = ph_fwd_cc(W, C, OW);
  VCG_CHECK_ARG(cc > 0, "vcg_patch_head_fwd: a map row of %d pixels does not fit the on-chip staging", W);
  VCG_CHECK_ARG(ws_bytes >= ph_fwd_ws(N, H, W, C, KH, KW), "vcg_patch_head_fwd: workspace too small");
  const int chunks = (C + cc - 1) / cc, groups = (N * OW + 16 * kPhFwdTiles - 1) / (16 * kPhFwdTiles);
  const size_t lds = ph_fwd_lds(N, W, OW, cc);
  hipStream_t st = (hipStream_t)stream;
  float* P = (float*)ws;
  const dim3 grid(chunks * ((KH + 15) / 16), H, groups);
  if (cc == 64)
    hipLaunchKernelGGL(k_ph_fwd<64>, grid, dim3(256), lds, st, x, wsn_k, P, N, H, W, C, KH, KW, OW, chunks);
  else if (cc == 32)
    hipLaunchKernelGGL(k_ph_fwd<32>, grid, dim3(256), lds, st, x, wsn_k, P, N, H, W, C, KH, KW, OW, chunks);
  else
    hipLaunchKernelGGL(k_ph_fwd<16>, grid, dim3(256), lds, st, x, wsn_k, P, N, H, W, C, KH, KW, OW, chunks);
  const size_t total = (size_t)N * OH * OW;
  hipLaunchKernelGGL(k_ph_fwd_sum, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, (const float*)P, bias, out, N, H, OH, OW,
                     KH, chunks);
  VCG_LAUNCH_CHECK("vcg_patch_head_fwd");
  return 0;
}

extern "C" int vcg_patch_head_dgrad(const float* g, const float* wsn_k, float* dx, int N, int H, int W, int C, int KH, int KW,
                                    void* stream) {
  VCG_CHECK_ARG(g && wsn_k && dx, "vcg_patch_head_dgrad: null pointer");
  VCG_CHECK_ARG(ph_dims_ok(N, H, W, C, KH, KW), "vcg_patch_head_dgrad: bad dims N %d map %dx%dx%d kernel %dx%d", N, C, H, W, KH, KW);
  const int OH = H - KH + 1, OW = W - KW + 1;
  const size_t lds = ph_dgrad_lds(N, W, KH, KW, OW);
  VCG_CHECK_ARG(lds <= (size_t)kPhLds, "vcg_patch_head_dgrad: a map row of %d pixels does not fit the on-chip staging", W);
  const int groups = (N * W + 16 * kPhDgTiles - 1) / (16 * kPhDgTiles);
  hipLaunchKernelGGL(k_ph_dgrad, dim3((C + 255) / 256, H, groups), dim3(256), lds, (hipStream_t)stream, g, wsn_k, dx, N, H, W, C,
                     KH, KW, OH, OW);
  VCG_LAUNCH_CHECK("vcg_patch_head_dgrad");
  return 0;
}

extern "C" int vcg_patch_head_wgrad(const float* g, const float* x, const float* wsn_k, const float* sigma, const float* u,
                                    const float* v, float* gw_orig_oihw, float* gbias, int N, int H, int W, int C, int KH, int KW,
                                    void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(g && x && wsn_k && sigma && u && v && gw_orig_oihw && ws, "vcg_patch_head_wgrad: null pointer");
  VCG_CHECK_ARG(ph_dims_ok(N, H, W, C, KH, KW), "vcg_patch_head_wgrad: bad dims N %d map %dx%dx%d kernel %dx%d", N, C, H, W, KH, KW);
  VCG_CHECK_ARG(ws_bytes >= ph_wgrad_ws(H, C, KH, KW), "vcg_patch_head_wgrad: workspace too small");
  const int OH = H - KH + 1, OW = W - KW + 1;
  const size_t K = (size_t)KH * KW * C;
  float* part = (float*)ws;
  float* gk = part + (size_t)H * K;
  float* pdot = gk + K;
  float* gsum = pdot + kPhRedBlocks;
  hipStream_t st = (hipStream_t)stream;
  const int kygroups = (KH + 3) / 4;
  hipLaunchKernelGGL(k_ph_wgrad, dim3(kygroups * ((KW + 15) / 16), (C + 255) / 256, H), dim3(256), 0, st, g, x, part, N, H, W, C, KH,
                     KW, OH, OW, kygroups);
  hipLaunchKernelGGL(k_ph_wgrad_sum, dim3(kPhRedBlocks), dim3(256), 0, st, (const float*)part, wsn_k, g, gk, pdot, gsum, K,
                     (size_t)KW * C, OH, (size_t)N * OH * OW);
  VCG_LAUNCH_CHECK("vcg_patch_head_wgrad");
  // the spectral-norm Jacobian, the OIHW permutation and gbias += (one addend: the logits' sum) are misc.hip's, unchanged
  return vcg_sn_wgrad_finish(gk, pdot, kPhRedBlocks, sigma, u, v, gsum, 1, gw_orig_oihw, gbias, C, KH * KW, st);
}
