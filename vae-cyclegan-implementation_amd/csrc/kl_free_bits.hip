// KL term of the variational models with a free-bits floor per latent channel (Kingma et al. 2016): a channel whose mean KL is
// at or below the floor stops being penalised, so no channel is driven to zero information.  Kernels of their own: the plain
// term (k_reduce_partial<1>, k_kl_bwd in misc.hip) is not touched, and a run without a floor launches none of these.
//
//   mu, lv: R x Cp fp32, the networks' NHWC buffers with R = N h w rows; C logical channels at pitch Cp (a multiple of 4), the
//   channel the fastest index.  Per element t = 1 + l - mu^2 - exp(l), l = clamp(lv, -10, 10) (the plain term's summand);
//   KL_c = -0.5 / R  sum over rows of t.
//
//   forward, two launches:
//     k_klfb_partial  a workgroup owns a slab of rows x a group of channel quads: lane (r, q) reads the float4 of quad q of its
//                     rows (lanes of one row are neighbours along the channel: coalesced), sums its rows in registers, and the
//                     TP row lanes of a quad are combined through LDS in a fixed tree.  One partial per (slab, channel).
//     k_klfb_final    one workgroup: per channel the slabs are summed in slab order in double, klc[c] = (float)KL_c, and the C
//                     channel results are reduced in a fixed order to out[0] = mean max(KL_c, floor), out[1] = mean KL_c,
//                     out[2] = the number of channels whose gate is open.
//   backward, one launch: k_klfb_bwd, grid-stride over float4s; the gate is recomputed from klc and floor, no mask is stored.
//
// The gate is decided on the fp32 klc[c] the forward wrote, by the same comparison in both directions: closed iff klc[c] <= floor
// (a tie is closed, a NaN leaves it open and reaches out[0] and out[1]).  Pad lanes c >= C are never summed into a result, never
// counted in C, and get gradient 0.  No atomics; every sum has a fixed order, so the same input gives the same bits.
#include <math.h>

#include "vcg_common.h"

#define KLFB_THREADS 256
#define KLFB_MAX_TC 64          // channel quads per workgroup (256 channels); the other lanes of the workgroup are row lanes
#define KLFB_MAX_SLABS 64       // the final launch reads at most this many partials per channel
#define KLFB_FINAL_THREADS 1024
#define KLFB_BWD_MAX_BLOCKS 2048

struct KlfbPlan {
  int tc, tp, cgroups;          // quads x row lanes of a workgroup (tc tp = 256, both powers of two), workgroups along the channel
  size_t slab, nslab;           // rows per workgroup (tp x rows per lane), workgroups along the rows (<= KLFB_MAX_SLABS)
};

static KlfbPlan klfb_plan(size_t rows, int cp) {
  KlfbPlan p;
  const int cp4 = cp / 4;
  int tc = 1;
  while (tc < cp4 && tc < KLFB_MAX_TC) tc *= 2;
  p.tc = tc;
  p.tp = KLFB_THREADS / tc;
  p.cgroups = (cp4 + tc - 1) / tc;
  const size_t per_round = (size_t)p.tp * KLFB_MAX_SLABS;
  size_t rpl = (rows + per_round - 1) / per_round;            // rows per lane
  if (rpl < 1) rpl = 1;
  p.slab = (size_t)p.tp * rpl;
  p.nslab = (rows + p.slab - 1) / p.slab;
  return p;
}

extern "C" size_t vcg_kl_fb_workspace(size_t rows, int cp) {
  if (rows == 0 || cp < 4 || cp % 4 != 0 || rows > ((size_t)1 << 40)) {
    vcg_set_error("vcg_kl_fb_workspace: bad arguments (rows %zu, cp %d)", rows, cp);
    return 0;
  }
  const KlfbPlan p = klfb_plan(rows, cp);
  return p.nslab * (size_t)cp * sizeof(float);
}

__device__ __forceinline__ float klfb_term(float mu, float lv) {
  const float l = fminf(fmaxf(lv, -10.f), 10.f);
  return 1.f + l - mu * mu - expf(l);
}

// grid (cgroups, nslab); part [nslab][cp]
__global__ __launch_bounds__(KLFB_THREADS) void k_klfb_partial(const float* __restrict__ mu, const float* __restrict__ lv,
                                                               float* __restrict__ part, size_t rows, int cp4, int tc,
                                                               int tc_log2, size_t slab) {
  __shared__ float4 red[KLFB_THREADS];
  const int tid = threadIdx.x, q = tid & (tc - 1), r = tid >> tc_log2, tp = KLFB_THREADS >> tc_log2;
  const int cq = blockIdx.x * tc + q;
  const size_t row0 = (size_t)blockIdx.y * slab;
  const size_t row1 = row0 + slab < rows ? row0 + slab : rows;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cq < cp4) {
    const float4* m4 = reinterpret_cast<const float4*>(mu);
    const float4* l4 = reinterpret_cast<const float4*>(lv);
    for (size_t row = row0 + r; row < row1; row += tp) {
      const float4 m = m4[row * cp4 + cq];
      const float4 l = l4[row * cp4 + cq];
      s.x += klfb_term(m.x, l.x);
      s.y += klfb_term(m.y, l.y);
      s.z += klfb_term(m.z, l.z);
      s.w += klfb_term(m.w, l.w);
    }
  }
  red[tid] = s;
  __syncthreads();
  for (int h = tp >> 1; h > 0; h >>= 1) {          // row lane r takes row lane r + h: the same tree for every input
    if (r < h) {
      const float4 o = red[tid + h * tc];
      s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
      red[tid] = s;
    }
    __syncthreads();
  }
  if (r == 0 && cq < cp4) reinterpret_cast<float4*>(part)[(size_t)blockIdx.y * cp4 + cq] = s;
}

__device__ __forceinline__ bool klfb_open(float kl, float floor_) { return !(kl <= floor_); }

// one workgroup; out3 = {floored mean, plain mean, open gates}
__global__ __launch_bounds__(KLFB_FINAL_THREADS) void k_klfb_final(const float* __restrict__ part, int nslab, int c, int cp,
                                                                   double scale, float floor_, float* __restrict__ klc,
                                                                   float* __restrict__ out3) {
  __shared__ double red[3][KLFB_FINAL_THREADS];
  double fl = 0.0, pl = 0.0, open = 0.0;
  for (int ch = threadIdx.x; ch < c; ch += KLFB_FINAL_THREADS) {
    double s = 0.0;
    int i = 0;
    for (; i + 8 <= nslab; i += 8) {              // eight loads in flight, added in slab order
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(i + j) * cp + ch];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (double)v[j];
    }
    for (; i < nslab; ++i) s += (double)part[(size_t)i * cp + ch];
    const float kl = (float)(s * scale);
    klc[ch] = kl;
    const bool o = klfb_open(kl, floor_);
    fl += o ? (double)kl : (double)floor_;
    pl += (double)kl;
    open += o ? 1.0 : 0.0;
  }
  red[0][threadIdx.x] = fl;
  red[1][threadIdx.x] = pl;
  red[2][threadIdx.x] = open;
  __syncthreads();
  for (int h = KLFB_FINAL_THREADS >> 1; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
      red[2][threadIdx.x] += red[2][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    const double v = red[threadIdx.x][0];
    out3[threadIdx.x] = (float)(threadIdx.x == 2 ? v : v / (double)c);
  }
}

static int klfb_check(const char* who, const float* mu, const float* lv, size_t rows, int c, int cp, float floor_) {
  VCG_CHECK_ARG(mu && lv, "%s: null pointer", who);
  VCG_CHECK_ARG(rows > 0 && rows <= ((size_t)1 << 40), "%s: rows must lie in 1..2^40, got %zu", who, rows);
  VCG_CHECK_ARG(c >= 1 && cp >= c && cp % 4 == 0, "%s: needs 1 <= c <= cp and cp a multiple of 4, got c %d, cp %d", who, c, cp);
  VCG_CHECK_ARG(isfinite(floor_) && floor_ >= 0.f, "%s: the floor must be finite and >= 0, got %g", who, (double)floor_);
  VCG_CHECK_ARG((((uintptr_t)mu | (uintptr_t)lv) & 15) == 0, "%s: mu or lv not 16-byte aligned", who);
  return 0;
}

extern "C" int vcg_kl_fb_fwd(const float* mu, const float* lv, float* out3, float* klc, size_t rows, int c, int cp, float floor_,
                             void* ws, size_t ws_bytes, void* stream) {
  if (klfb_check("vcg_kl_fb_fwd", mu, lv, rows, c, cp, floor_)) return -1;
  VCG_CHECK_ARG(out3 && klc && ws, "vcg_kl_fb_fwd: null pointer");
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_kl_fb_fwd: workspace not 16-byte aligned");
  const KlfbPlan p = klfb_plan(rows, cp);
  VCG_CHECK_ARG(ws_bytes >= p.nslab * (size_t)cp * sizeof(float), "vcg_kl_fb_fwd: workspace too small (%zu bytes, needs %zu)",
                ws_bytes, p.nslab * (size_t)cp * sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  int tc_log2 = 0;
  while ((1 << tc_log2) < p.tc) ++tc_log2;
  hipLaunchKernelGGL(k_klfb_partial, dim3(p.cgroups, (unsigned)p.nslab), dim3(KLFB_THREADS), 0, st, mu, lv, (float*)ws, rows,
                     cp / 4, p.tc, tc_log2, p.slab);
  hipLaunchKernelGGL(k_klfb_final, dim3(1), dim3(KLFB_FINAL_THREADS), 0, st, (const float*)ws, (int)p.nslab, c, cp,
                     -0.5 / (double)rows, floor_, klc, out3);
  VCG_LAUNCH_CHECK("vcg_kl_fb_fwd");
  return 0;
}

// n4 = rows cp4 float4s; s = gout / (R C) where the channel's gate is open, else 0
template <typename IDX>
__global__ __launch_bounds__(KLFB_THREADS) void k_klfb_bwd(const float* __restrict__ mu, const float* __restrict__ lv,
                                                           const float* __restrict__ gout, const float* __restrict__ klc,
                                                           float* __restrict__ gmu, float* __restrict__ glv, IDX n4, IDX cp4, int c,
                                                           float floor_, float inv_rc) {
  const float s = gout[0] * inv_rc;
  for (IDX i = (IDX)blockIdx.x * KLFB_THREADS + threadIdx.x; i < n4; i += (IDX)gridDim.x * KLFB_THREADS) {
    const int c0 = (int)(i % cp4) * 4;
    const float4 m = reinterpret_cast<const float4*>(mu)[i];
    const float4 l = reinterpret_cast<const float4*>(lv)[i];
    const float mv[4] = {m.x, m.y, m.z, m.w}, lvv[4] = {l.x, l.y, l.z, l.w};
    float gm[4], gl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ch = c0 + j;
      const float sc = (ch < c && klfb_open(klc[ch < c ? ch : 0], floor_)) ? s : 0.f;
      const bool live = ch < c && sc != 0.f;          // a closed gate or a pad lane: exactly 0, whatever mu and lv hold
      const float lc = fminf(fmaxf(lvv[j], -10.f), 10.f);
      gm[j] = live ? mv[j] * sc : 0.f;
      gl[j] = (live && lvv[j] >= -10.f && lvv[j] <= 10.f) ? -0.5f * (1.f - expf(lc)) * sc : 0.f;
    }
    reinterpret_cast<float4*>(gmu)[i] = make_float4(gm[0], gm[1], gm[2], gm[3]);
    reinterpret_cast<float4*>(glv)[i] = make_float4(gl[0], gl[1], gl[2], gl[3]);
  }
}

extern "C" int vcg_kl_fb_bwd(const float* mu, const float* lv, const float* gout, const float* klc, float* gmu, float* glv,
                             size_t rows, int c, int cp, float floor_, void* stream) {
  if (klfb_check("vcg_kl_fb_bwd", mu, lv, rows, c, cp, floor_)) return -1;
  VCG_CHECK_ARG(gout && klc && gmu && glv, "vcg_kl_fb_bwd: null pointer");
  VCG_CHECK_ARG((((uintptr_t)gmu | (uintptr_t)glv) & 15) == 0, "vcg_kl_fb_bwd: gmu or glv not 16-byte aligned");
  const size_t cp4 = (size_t)cp / 4, n4 = rows * cp4;
  size_t blocks = (n4 + KLFB_THREADS - 1) / KLFB_THREADS;
  if (blocks > KLFB_BWD_MAX_BLOCKS) blocks = KLFB_BWD_MAX_BLOCKS;
  const float inv_rc = 1.0f / (float)(rows * (size_t)c);          // vcg_kl_bwd's 1 / n: an all-open step has the plain term's bits
  hipStream_t st = (hipStream_t)stream;
  if (n4 + (size_t)KLFB_BWD_MAX_BLOCKS * KLFB_THREADS < ((size_t)1 << 32))      // the loop index cannot wrap in 32 bits
    hipLaunchKernelGGL(k_klfb_bwd<uint32_t>, dim3((unsigned)blocks), dim3(KLFB_THREADS), 0, st, mu, lv, gout, klc, gmu, glv,
                       (uint32_t)n4, (uint32_t)cp4, c, floor_, inv_rc);
  else
    hipLaunchKernelGGL(k_klfb_bwd<size_t>, dim3((unsigned)blocks), dim3(KLFB_THREADS), 0, st, mu, lv, gout, klc, gmu, glv, n4, cp4,
                       c, floor_, inv_rc);
  VCG_LAUNCH_CHECK("vcg_kl_fb_bwd");
  return 0;
}
