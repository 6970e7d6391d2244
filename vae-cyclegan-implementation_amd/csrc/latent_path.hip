// The interpolating translator (translate.py --interpolate N): the path through latent space between consecutive frames.
// New: the reference has no inference path.
//
//   vcg_latent_pair_stats  sum a^2, sum b^2, sum a b of each pair (a[p], b[p]) of latent maps over the LOGICAL channels, every
//                          summand and sum in double.  A lane strides over the pair's float4 quads; the 64 lanes of a wavefront are
//                          combined by a butterfly of shuffles, the wavefronts through LDS in wavefront order; each workgroup
//                          writes its partial to a slot of its own and a final launch sums a pair's slots in a fixed order
//                          (metrics.hip's scheme): no atomics.  The number of workgroups of a pair is a function of `per` alone,
//                          so a pair's three numbers do not depend on P or on the other pairs of the call.
//   vcg_latent_path        z[(p, j)] = ca(p, j) a[p] + cb(p, j) b[p] for a chunk j = first .. first + k - 1 of the T uniform
//                          fractions t_j = j / (T - 1).  A workgroup stages the coefficient pairs of its pair in LDS (each
//                          evaluated in double from the pair's stats and rounded once; every workgroup runs the same code on the
//                          same numbers, so they all hold the same bits), then every lane loads its float4 of a and of b ONCE and
//                          walks the fractions with them in registers: (2 + k) per floats of traffic per pair, not 3 k per.
//                          j == 0 and j == T - 1 store the loaded bits of a and b.  Elsewhere z = fmaf(ca, a, __fmul_rn(cb, b)):
//                          one sequence whatever the chunking, and the file is compiled with contraction off.
//
// a and b are only read, so they may overlap (mu and mu + per: the consecutive frames of one encoder batch); z may not overlap
// either.  Pad lanes (channels C .. pitch - 1 of a pixel) are loaded with their quad but selected out before any arithmetic: a
// NaN there reaches neither a sum nor z, whose pad lanes are written as 0.
#include <math.h>

#include "vcg_common.h"

#pragma clang fp contract(off)

#define LP_THREADS 256
#define LP_WAVES (LP_THREADS / 64)
#define LP_STATS_BLOCKS 128      // workgroups per pair of the stats, at most: the slots the final pass sums
#define LP_PATH_BLOCKS 256       // workgroups per pair of the path, at most
#define LP_KTILE 256             // fractions whose coefficients are staged at a time
#define LP_MAX_GRID_Y 65535

static inline bool lp_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// workgroups over the per4 quads of one pair: a function of per4 alone
static int lp_blocks(size_t per4, int cap) {
  size_t b = (per4 + LP_THREADS - 1) / LP_THREADS;
  if (b > (size_t)cap) b = (size_t)cap;
  if (b < 1) b = 1;
  return (int)b;
}

// how many of the four lanes of quad q are logical channels (the pitch is pitch4 quads; q < per4 <= 2^29: a 32-bit remainder)
__device__ __forceinline__ int lp_valid(size_t q, uint32_t pitch4, int C) {
  const int left = C - 4 * (int)((uint32_t)q % pitch4);
  return left < 0 ? 0 : (left > 4 ? 4 : left);
}

// ---------------------------------------------------------------- sum a^2, sum b^2, sum a b per pair
// grid (blocks over per4, pairs); ws[(p nblk + block) 3 + s].  The product of two fp32 values is exact in double.
__global__ __launch_bounds__(LP_THREADS) void k_latent_pair_stats(const float4* a, const float4* b, double* __restrict__ ws, size_t per4,
                                                                  uint32_t pitch4, int C, int P) {
  __shared__ double red[3][LP_WAVES];
  const int tid = threadIdx.x;
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    const float4* ap = a + (size_t)p * per4;
    const float4* bp = b + (size_t)p * per4;
    double saa = 0.0, sbb = 0.0, sab = 0.0;
    for (size_t q = (size_t)blockIdx.x * LP_THREADS + tid; q < per4; q += (size_t)gridDim.x * LP_THREADS) {
      const float4 va = ap[q], vb = bp[q];
      const int valid = lp_valid(q, pitch4, C);
      const float av[4] = {va.x, va.y, va.z, va.w}, bv[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < valid) {                          // a select, not a product with 0: a NaN pad lane stays out
          const double x = (double)av[c], y = (double)bv[c];
          saa += x * x;
          sbb += y * y;
          sab += x * y;
        }
      }
    }
    saa = wave_sum_d(saa);
    sbb = wave_sum_d(sbb);
    sab = wave_sum_d(sab);
    __syncthreads();                              // the previous pair's sums have been read
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = saa;
      red[1][tid >> 6] = sbb;
      red[2][tid >> 6] = sab;
    }
    __syncthreads();
    if (tid < 3) {                                // lane s finishes sum s: wavefront order
      double v = red[tid][0];
#pragma unroll
      for (int w = 1; w < LP_WAVES; ++w) v += red[tid][w];
      ws[((size_t)p * gridDim.x + blockIdx.x) * 3 + tid] = v;
    }
  }
}

// one wavefront per pair: lane l sums the slots l, l + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void k_latent_pair_stats_final(const double* __restrict__ ws, double* __restrict__ out, int nblk) {
  const size_t p = blockIdx.x;
  const double* slots = ws + p * (size_t)nblk * 3;
  for (int s = 0; s < 3; ++s) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) v += slots[(size_t)i * 3 + s];
    v = wave_sum_d(v);
    if (threadIdx.x == 0) out[p * 3 + s] = v;
  }
}

static bool lp_layout_ok(const char* who, int P, size_t per, int C, int pitch) {
  if (P < 1) {
    vcg_set_error("%s: P=%d must be at least 1", who, P);
    return false;
  }
  if (per == 0 || per > ((size_t)1 << 31)) {
    vcg_set_error("%s: per=%zu must be in 1 .. 2^31", who, per);
    return false;
  }
  if (pitch < 4 || pitch % 4 != 0 || C < 1 || C > pitch || per % (size_t)pitch != 0) {
    vcg_set_error("%s: C=%d, pitch=%d, per=%zu: the pitch must be a multiple of 4 that holds the C >= 1 channels and divides per", who,
                  C, pitch, per);
    return false;
  }
  return true;
}

extern "C" size_t vcg_latent_stats_workspace(int P, size_t per) {
  if (P < 1 || per == 0 || per % 4 != 0 || per > ((size_t)1 << 31)) {
    vcg_set_error("vcg_latent_stats_workspace: bad P=%d per=%zu", P, per);
    return 0;
  }
  return ((size_t)P * lp_blocks(per / 4, LP_STATS_BLOCKS) * 3 * sizeof(double) + 15) / 16 * 16;
}

extern "C" int vcg_latent_pair_stats(const float* a, const float* b, double* out, int P, size_t per, int C, int pitch, void* ws,
                                     size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(a && b && out && ws, "vcg_latent_pair_stats: null pointer");
  if (!lp_layout_ok("vcg_latent_pair_stats", P, per, C, pitch)) return -1;
  VCG_CHECK_ARG(lp_aligned(a, 16) && lp_aligned(b, 16) && lp_aligned(out, 8) && lp_aligned(ws, 8),
                "vcg_latent_pair_stats: a and b must be 16-byte aligned, out and ws 8-byte aligned");
  const size_t need = vcg_latent_stats_workspace(P, per);
  VCG_CHECK_ARG(need != 0 && ws_bytes >= need, "vcg_latent_pair_stats: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const size_t per4 = per / 4;
  const int nblk = lp_blocks(per4, LP_STATS_BLOCKS);
  hipLaunchKernelGGL(k_latent_pair_stats, dim3(nblk, P < LP_MAX_GRID_Y ? P : LP_MAX_GRID_Y), dim3(LP_THREADS), 0, (hipStream_t)stream,
                     (const float4*)a, (const float4*)b, (double*)ws, per4, (uint32_t)(pitch / 4), C, P);
  hipLaunchKernelGGL(k_latent_pair_stats_final, dim3(P), dim3(64), 0, (hipStream_t)stream, (const double*)ws, out, nblk);
  VCG_LAUNCH_CHECK("vcg_latent_pair_stats");
  return 0;
}

// ---------------------------------------------------------------- the path
struct LatentPathP {
  const float4* a;        // (P, per4) quads; a and b may overlap
  const float4* b;
  const double* stats;    // (P, 3) of vcg_latent_pair_stats; not read by the lerp
  float4* z;              // (P, k, per4)
  float2* coef_out;       // (P, k) pairs (ca, cb), or null
  size_t per4;
  uint32_t pitch4;
  int C, P, T, first, k, mode;
};

// (ca, cb) of fraction j of T for a pair with stats st: evaluated in double, rounded once.  A NaN or infinite stat fails every
// comparison below and leaves the lerp coefficients.
__device__ float2 lp_coef(int j, int T, int mode, const double* st) {
  const double t = (double)j / (double)(T - 1);
  double ca = 1.0 - t, cb = t;
  if (mode == VCG_LATENT_SLERP) {
    const double saa = st[0], sbb = st[1], sab = st[2];
    if (saa > 0.0 && sbb > 0.0) {
      double c = sab / sqrt(saa * sbb);
      c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
      const double w = acos(c), sw = sin(w);
      if (sw >= VCG_SLERP_MIN_SIN) {
        ca = sin((1.0 - t) * w) / sw;
        cb = sin(t * w) / sw;
      }
    }
  }
  return make_float2((float)ca, (float)cb);
}

__device__ __forceinline__ float lp_blend(float2 c, float a, float b) { return fmaf(c.x, a, __fmul_rn(c.y, b)); }

// grid (blocks over per4, pairs)
__global__ __launch_bounds__(LP_THREADS) void k_latent_path(LatentPathP p) {
  __shared__ float2 coef[LP_KTILE];
  const int tid = threadIdx.x;
  const int last = p.T - 1;
  for (int pr = blockIdx.y; pr < p.P; pr += gridDim.y) {
    const float4* ap = p.a + (size_t)pr * p.per4;
    const float4* bp = p.b + (size_t)pr * p.per4;
    for (int k0 = 0; k0 < p.k; k0 += LP_KTILE) {
      const int kt = p.k - k0 < LP_KTILE ? p.k - k0 : LP_KTILE;
      __syncthreads();                            // the previous tile's coefficients have been read
      if (tid < kt) {
        const float2 c = lp_coef(p.first + k0 + tid, p.T, p.mode, p.stats + (size_t)pr * 3);
        coef[tid] = c;
        if (p.coef_out && blockIdx.x == 0) p.coef_out[(size_t)pr * p.k + k0 + tid] = c;
      }
      __syncthreads();
      float4* zp = p.z + ((size_t)pr * p.k + k0) * p.per4;
      for (size_t q = (size_t)blockIdx.x * LP_THREADS + tid; q < p.per4; q += (size_t)gridDim.x * LP_THREADS) {
        float4 va = ap[q], vb = bp[q];
        const int valid = lp_valid(q, p.pitch4, p.C);
        if (valid < 4) {                          // pad lanes: 0 in every fraction, the endpoints included
          va.w = 0.f; vb.w = 0.f;
          if (valid < 3) { va.z = 0.f; vb.z = 0.f; }
          if (valid < 2) { va.y = 0.f; vb.y = 0.f; }
          if (valid < 1) { va.x = 0.f; vb.x = 0.f; }
        }
        for (int jj = 0; jj < kt; ++jj) {
          const int j = p.first + k0 + jj;
          float4 o;
          if (j == 0) {
            o = va;
          } else if (j == last) {
            o = vb;
          } else {
            const float2 c = coef[jj];            // one address for the whole wavefront: a broadcast
            o = make_float4(lp_blend(c, va.x, vb.x), lp_blend(c, va.y, vb.y), lp_blend(c, va.z, vb.z), lp_blend(c, va.w, vb.w));
          }
          zp[(size_t)jj * p.per4 + q] = o;
        }
      }
    }
  }
}

extern "C" int vcg_latent_path(const float* a, const float* b, const double* stats, float* z, float* coef_out, int P, int T, int first,
                               int k, size_t per, int C, int pitch, int mode, void* stream) {
  VCG_CHECK_ARG(mode == VCG_LATENT_SLERP || mode == VCG_LATENT_LERP, "vcg_latent_path: unknown mode %d", mode);
  VCG_CHECK_ARG(a && b && z && (stats || mode == VCG_LATENT_LERP), "vcg_latent_path: null pointer");
  if (!lp_layout_ok("vcg_latent_path", P, per, C, pitch)) return -1;
  VCG_CHECK_ARG(T >= 2, "vcg_latent_path: T=%d: a path has at least its two endpoints", T);
  VCG_CHECK_ARG(k >= 1 && first >= 0 && (long long)first + k <= T, "vcg_latent_path: fractions %d .. %lld leave the %d of the path", first,
                (long long)first + k - 1, T);
  VCG_CHECK_ARG(lp_aligned(a, 16) && lp_aligned(b, 16) && lp_aligned(z, 16) && lp_aligned(stats, 8) && lp_aligned(coef_out, 8),
                "vcg_latent_path: a, b and z must be 16-byte aligned, stats and coef_out 8-byte aligned");
  LatentPathP p;
  p.a = (const float4*)a; p.b = (const float4*)b; p.stats = stats; p.z = (float4*)z; p.coef_out = (float2*)coef_out;
  p.per4 = per / 4; p.pitch4 = (uint32_t)(pitch / 4);
  p.C = C; p.P = P; p.T = T; p.first = first; p.k = k; p.mode = mode;
  hipLaunchKernelGGL(k_latent_path, dim3(lp_blocks(p.per4, LP_PATH_BLOCKS), P < LP_MAX_GRID_Y ? P : LP_MAX_GRID_Y), dim3(LP_THREADS), 0,
                     (hipStream_t)stream, p);
  VCG_LAUNCH_CHECK("vcg_latent_path");
  return 0;
}
