// Sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al., ICLR 2018, section 5): the evaluator's score for
// unpaired runs.  It compares the patch statistics of a set of generated images with a set of real ones, level by level of a
// Laplacian pyramid, and needs neither pairing nor a pretrained network.  Forward only: a metric, not a loss.  DESIGN.md,
// "Sliced Wasserstein distance", has the definition; the stages, in the order a level goes through them:
//
// k_swd_pyramid   one level of the pyramid from the physical (N, S, S, 4) buffer.  g = [1, 4, 6, 4, 1] / 16, K = g (x) g, borders
//                 mirrored without repeating the edge (reflect_idx).  down(I)[i, j] = (K * I)[2i, 2j]; up(J) = (4 K) * Z with
//                 Z[2i, 2j] = J[i, j] and 0 elsewhere; G' = down(G), L = G - up(G').  One workgroup per 32 x 32 tile of G: it
//                 stages the tile with a halo of 4 above / left and 3 below / right in LDS (one float4 load per pixel, `clamp01`
//                 on level 0), forms the 18 x 18 values of G' that up() needs for the tile there — each at its true (mirrored)
//                 index and with the taps in one order, so they are the bits the owning workgroup writes to HBM — writes its own
//                 16 x 16 of them as G' and the tile of L.  G is read from HBM once.  The weights are multiples of 1 / 256: the
//                 only roundings are those of the fp32 sums.  Channel 3 of both outputs is 0.
// k_swd_gather    row d of the (rows, 147) descriptor matrix = the 7 x 7 x 3 patch of plan entry d, flattened (c, dy, dx).  The
//                 plan (image, top, left) is drawn on the host and travels in the kernel arguments, SWD_PLAN_CHUNK entries per
//                 launch: nothing is uploaded or synchronised.
// k_swd_sum<P>    channel statistics over all rows and the 49 patch pixels of a channel, in double.  Workgroup b sums the rows
//                 [b SWD_STAT_ROWS, (b + 1) SWD_STAT_ROWS) column by column, then the 49 columns of a channel in order, into its
//                 own three slots.  P = 0: sums of x; P = 1: sums of (x - mean)^2 with the mean taken from the P = 0 slots in a
//                 fixed order (two passes: a constant channel gives a deviation of exactly 0, so its level is non-finite and the
//                 caller reports it as missing, instead of the garbage a cancelling E[x^2] - mean^2 would give).
// k_swd_norm      (x - mean) / sqrt(sum of squares / count), evaluated in double and rounded once.
// k_swd_project   out[j][r] = sum_k dirs[k][j] desc[r][k]: the (ndir, n) TRANSPOSE of desc x dirs, so that the column a sort
//                 workgroup owns is contiguous.  fp32 products and fp32 accumulation on v_mfma_f32_32x32x2_f32 (freq_loss.hip's
//                 tile: 256 threads, 64 x 64 outputs, K staged 32 at a time with zero fill).
// k_sort_columns  bitonic sort of one column per workgroup in LDS, ascending.  The n keys are padded with +inf to the next
//                 power of two P <= 16384 (64 KiB).  Every loop bound is a function of P: a NaN key (it compares false both
//                 ways and never moves its partner) can neither stall the network nor send an index out of range; its column
//                 simply comes out unsorted.  The matrix is addressed with a row and a column stride, so the transposed
//                 projections and a plain (n, cols) matrix take the same kernel.
// k_swd_dist      mean |a - b| over two equally laid out arrays, in double: workgroup b sums a chunk into its own slot,
//                 k_swd_dist_final adds the slots in a fixed order.
// No float atomics anywhere: the same input gives the same bits.
#include <math.h>

#include "vcg_common.h"

#define SWD_TILE 32
#define SWD_HALO_LO 4
#define SWD_STAGE (SWD_TILE + 7)          // 39: G rows y0 - 4 .. y0 + 34
#define SWD_JT (SWD_TILE / 2 + 2)         // 18: G' rows y0 / 2 - 1 .. y0 / 2 + 16
#define SWD_PATCH 7
#define SWD_DESC (3 * SWD_PATCH * SWD_PATCH)      // 147
#define SWD_PLAN_CHUNK 256
#define SWD_STAT_ROWS 256
#define SWD_STAT_THREADS 192
#define SWD_MAX_STAT_BLOCKS (VCG_SWD_MAX_DESC / SWD_STAT_ROWS)      // 64
#define SWD_SORT_THREADS 512
#define SWD_DIST_CHUNK 8192
#define SWD_DIST_MAX_BLOCKS 4096

// ---- pyramid ----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float swd_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }      // a NaN stays

struct SwdPyrP {
  const float4* g;       // (N, S, S, 4)
  float4* gnext;         // (N, S / 2, S / 2, 4), or null: no coarser level, lap = G
  float4* lap;           // (N, S, S, 4)
  int S, clamp;
};

__global__ __launch_bounds__(256) void k_swd_pyramid(SwdPyrP p) {
  __shared__ float sg[3][SWD_STAGE * SWD_STAGE];
  __shared__ float sj[3][SWD_JT * SWD_JT];
  const int tid = threadIdx.x, S = p.S, n = blockIdx.z, y0 = blockIdx.y * SWD_TILE, x0 = blockIdx.x * SWD_TILE;
  const size_t img = (size_t)n * S * S;
  // G at the positions (y0 - 4 + r, x0 - 4 + c), mirrored into the image; positions past S + 1 are never used (and reflect_idx
  // does not cover them): 0
  for (int i = tid; i < SWD_STAGE * SWD_STAGE; i += 256) {
    const int r = i / SWD_STAGE, c = i - r * SWD_STAGE, y = y0 - SWD_HALO_LO + r, x = x0 - SWD_HALO_LO + c;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y <= S + 1 && x <= S + 1) {
      v = p.g[img + (size_t)reflect_idx(y, S) * S + reflect_idx(x, S)];
      if (p.clamp) { v.x = swd_clamp01(v.x); v.y = swd_clamp01(v.y); v.z = swd_clamp01(v.z); }
    }
    sg[0][i] = v.x; sg[1][i] = v.y; sg[2][i] = v.z;
  }
  __syncthreads();
  const float g5[5] = {1.f / 16, 4.f / 16, 6.f / 16, 4.f / 16, 1.f / 16};
  if (p.gnext) {
    // Z row 2 (j0 - 1 + a), a < 18, is row ri = reflect(2 (j0 - 1 + a)) / 2 of G' (S is even: the mirror keeps the parity), whose
    // taps are the G rows 2 ri - 2 .. 2 ri + 2: staged rows within y0 - 4 .. min(y0 + 34, S)
    const int S2 = S >> 1, j0 = y0 >> 1, i0 = x0 >> 1;
    for (int i = tid; i < SWD_JT * SWD_JT; i += 256) {
      const int a = i / SWD_JT, b = i - a * SWD_JT, zy = 2 * (j0 - 1 + a), zx = 2 * (i0 - 1 + b);
      float acc[3] = {0.f, 0.f, 0.f};
      if (zy <= S && zx <= S) {
        const int ry = reflect_idx(zy, S), rx = reflect_idx(zx, S);
        const int ly = ry - 2 - (y0 - SWD_HALO_LO), lx = rx - 2 - (x0 - SWD_HALO_LO);      // 0 .. 34
#pragma unroll
        for (int dy = 0; dy < 5; ++dy)
#pragma unroll
          for (int dx = 0; dx < 5; ++dx) {
            const float w = g5[dy] * g5[dx];
            const int o = (ly + dy) * SWD_STAGE + lx + dx;
            acc[0] = fmaf(w, sg[0][o], acc[0]);
            acc[1] = fmaf(w, sg[1][o], acc[1]);
            acc[2] = fmaf(w, sg[2][o], acc[2]);
          }
        // the workgroup's own 16 x 16 values of G' (there the mirror is the identity)
        const int iy = j0 - 1 + a, ix = i0 - 1 + b;
        if (a >= 1 && a <= SWD_TILE / 2 && b >= 1 && b <= SWD_TILE / 2 && iy < S2 && ix < S2)
          p.gnext[((size_t)n * S2 + iy) * S2 + ix] = make_float4(acc[0], acc[1], acc[2], 0.f);
      }
      sj[0][i] = acc[0]; sj[1][i] = acc[1]; sj[2][i] = acc[2];
    }
    __syncthreads();
  }
  for (int i = tid; i < SWD_TILE * SWD_TILE; i += 256) {
    const int r = i / SWD_TILE, c = i - r * SWD_TILE, y = y0 + r, x = x0 + c;
    if (y >= S || x >= S) continue;
    const int o = (r + SWD_HALO_LO) * SWD_STAGE + c + SWD_HALO_LO;
    float up[3] = {0.f, 0.f, 0.f};
    if (p.gnext) {
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy) {
        const int zy = y + dy;
        if (zy & 1) continue;
        const int a = (zy >> 1) - ((y0 >> 1) - 1);           // zy >= y0 - 2: a >= 0; zy <= y0 + 33: a <= 17
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
          const int zx = x + dx;
          if (zx & 1) continue;
          const int b = (zx >> 1) - ((x0 >> 1) - 1);
          const float w = 4.f * g5[dy + 2] * g5[dx + 2];
          const int q = a * SWD_JT + b;
          up[0] = fmaf(w, sj[0][q], up[0]);
          up[1] = fmaf(w, sj[1][q], up[1]);
          up[2] = fmaf(w, sj[2][q], up[2]);
        }
      }
    }
    p.lap[img + (size_t)y * S + x] = make_float4(sg[0][o] - up[0], sg[1][o] - up[1], sg[2][o] - up[2], 0.f);
  }
}

extern "C" int vcg_swd_pyramid_level(const float* g, float* g_next, float* lap, int N, int S, int clamp, void* stream) {
  VCG_CHECK_ARG(g && lap, "vcg_swd_pyramid_level: null pointer");
  VCG_CHECK_ARG(N > 0 && N <= 65535, "vcg_swd_pyramid_level: bad N=%d", N);
  VCG_CHECK_ARG(S >= 8 && S <= 32768, "vcg_swd_pyramid_level: bad S=%d (8 .. 32768)", S);
  VCG_CHECK_ARG(!g_next || (S & 1) == 0, "vcg_swd_pyramid_level: S=%d is odd: it has no coarser level", S);
  VCG_CHECK_ARG((((uintptr_t)g | (uintptr_t)g_next | (uintptr_t)lap) & 15) == 0, "vcg_swd_pyramid_level: images not 16-byte aligned");
  VCG_CHECK_ARG(g != lap && g != g_next && lap != g_next, "vcg_swd_pyramid_level: the buffers must be distinct");
  SwdPyrP p;
  p.g = (const float4*)g; p.gnext = (float4*)g_next; p.lap = (float4*)lap; p.S = S; p.clamp = clamp != 0;
  const int tiles = (S + SWD_TILE - 1) / SWD_TILE;
  hipLaunchKernelGGL(k_swd_pyramid, dim3(tiles, tiles, N), dim3(256), 0, (hipStream_t)stream, p);
  VCG_LAUNCH_CHECK("vcg_swd_pyramid_level");
  return 0;
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------

struct SwdPlanChunk { int32_t e[SWD_PLAN_CHUNK][3]; };      // (image, top, left)

__global__ __launch_bounds__(SWD_STAT_THREADS) void k_swd_gather(SwdPlanChunk plan, const float* __restrict__ lvl, int S,
                                                                 float* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= SWD_DESC) return;
  const int d = blockIdx.x, c = t / 49, rem = t - 49 * c, dy = rem / 7, dx = rem - 7 * dy;
  const int n = plan.e[d][0], top = plan.e[d][1], left = plan.e[d][2];
  out[(size_t)d * SWD_DESC + t] = lvl[(((size_t)n * S + top + dy) * S + left + dx) * 4 + c];
}

extern "C" int vcg_swd_gather(const float* level, int N, int S, const int32_t* plan, int count, float* out, size_t row_offset,
                              size_t rows, void* stream) {
  VCG_CHECK_ARG(level && out && (plan || count == 0), "vcg_swd_gather: null pointer");
  VCG_CHECK_ARG(N > 0 && S >= SWD_PATCH && S <= 32768, "vcg_swd_gather: bad N=%d S=%d", N, S);
  VCG_CHECK_ARG(count >= 0, "vcg_swd_gather: bad count=%d", count);
  VCG_CHECK_ARG(row_offset <= rows && (size_t)count <= rows - row_offset,
                "vcg_swd_gather: rows %zu .. %zu leave the matrix of %zu rows", row_offset, row_offset + (size_t)count, rows);
  VCG_CHECK_ARG((((uintptr_t)level | (uintptr_t)out) & 3) == 0, "vcg_swd_gather: pointers not 4-byte aligned");
  for (int d = 0; d < count; ++d) {
    const int32_t* e = plan + 3 * (size_t)d;
    VCG_CHECK_ARG(e[0] >= 0 && e[0] < N && e[1] >= 0 && e[1] <= S - SWD_PATCH && e[2] >= 0 && e[2] <= S - SWD_PATCH,
                  "vcg_swd_gather: plan entry %d = (%d, %d, %d) leaves the %d images of %dx%d", d, e[0], e[1], e[2], N, S, S);
  }
  static_assert(sizeof(SwdPlanChunk) <= 3072, "the plan chunk must fit the kernel arguments");
  SwdPlanChunk chunk;             // the launch copies it into the kernel arguments before it returns
  memset(&chunk, 0, sizeof(chunk));
  for (int d0 = 0; d0 < count; d0 += SWD_PLAN_CHUNK) {
    const int m = count - d0 < SWD_PLAN_CHUNK ? count - d0 : SWD_PLAN_CHUNK;
    memcpy(chunk.e, plan + 3 * (size_t)d0, (size_t)m * 3 * sizeof(int32_t));
    hipLaunchKernelGGL(k_swd_gather, dim3(m), dim3(SWD_STAT_THREADS), 0, (hipStream_t)stream, chunk, level, S,
                       out + (row_offset + d0) * SWD_DESC);
  }
  VCG_LAUNCH_CHECK("vcg_swd_gather");
  return 0;
}

// ---- channel statistics and normalisation ---------------------------------------------------------------------------------------

struct SwdStatP {
  const float* x;        // (n, 147)
  float* out;            // (n, 147); may be x
  double* sum;           // [blocks][3]
  double* sq;            // [blocks][3]
  int n, blocks;
};

// the three channel sums of `slots`, blocks in order
__device__ __forceinline__ double swd_slot_total(const double* slots, int blocks, int c) {
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += slots[3 * b + c];
  return s;
}

template <int PASS>
__global__ __launch_bounds__(SWD_STAT_THREADS) void k_swd_sum(SwdStatP p) {
  __shared__ double col[SWD_DESC];
  const int t = threadIdx.x, r0 = blockIdx.x * SWD_STAT_ROWS;
  const int r1 = r0 + SWD_STAT_ROWS < p.n ? r0 + SWD_STAT_ROWS : p.n;
  if (t < SWD_DESC) {
    double mean = 0.0;
    if (PASS == 1) mean = swd_slot_total(p.sum, p.blocks, t / 49) / ((double)p.n * 49.0);
    double s = 0.0;
    for (int r = r0; r < r1; ++r) {
      const double d = (double)p.x[(size_t)r * SWD_DESC + t] - mean;
      s += PASS == 0 ? d : d * d;
    }
    col[t] = s;
  }
  __syncthreads();
  if (t < 3) {
    double s = 0.0;
    for (int k = 0; k < 49; ++k) s += col[49 * t + k];
    (PASS == 0 ? p.sum : p.sq)[3 * blockIdx.x + t] = s;
  }
}

__global__ __launch_bounds__(SWD_STAT_THREADS) void k_swd_norm(SwdStatP p) {
  __shared__ double smean[3], sstd[3];
  const int t = threadIdx.x, r0 = blockIdx.x * SWD_STAT_ROWS;
  const int r1 = r0 + SWD_STAT_ROWS < p.n ? r0 + SWD_STAT_ROWS : p.n;
  if (t < 3) {
    const double cnt = (double)p.n * 49.0;
    smean[t] = swd_slot_total(p.sum, p.blocks, t) / cnt;
    sstd[t] = sqrt(swd_slot_total(p.sq, p.blocks, t) / cnt);
  }
  __syncthreads();
  if (t >= SWD_DESC) return;
  const double mean = smean[t / 49], sd = sstd[t / 49];
  for (int r = r0; r < r1; ++r) {
    const size_t at = (size_t)r * SWD_DESC + t;
    p.out[at] = (float)(((double)p.x[at] - mean) / sd);      // sd == 0: 0 / 0, the level is non-finite
  }
}

static int swd_rows_ok(const char* who, int n) {
  VCG_CHECK_ARG(n >= 1 && n <= VCG_SWD_MAX_DESC, "%s: %d descriptors (1 .. %d)", who, n, VCG_SWD_MAX_DESC);
  return 0;
}

extern "C" size_t vcg_swd_normalize_workspace(int n) {
  if (swd_rows_ok("vcg_swd_normalize_workspace", n) != 0) return 0;
  return (size_t)SWD_MAX_STAT_BLOCKS * 3 * 2 * sizeof(double);
}

extern "C" int vcg_swd_normalize(const float* desc, float* out, int n, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(desc && out && ws, "vcg_swd_normalize: null pointer");
  if (swd_rows_ok("vcg_swd_normalize", n) != 0) return -1;
  VCG_CHECK_ARG(ws_bytes >= vcg_swd_normalize_workspace(n), "vcg_swd_normalize: workspace of %zu bytes, %zu needed", ws_bytes,
                vcg_swd_normalize_workspace(n));
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_swd_normalize: workspace not 16-byte aligned");
  VCG_CHECK_ARG((((uintptr_t)desc | (uintptr_t)out) & 3) == 0, "vcg_swd_normalize: matrices not 4-byte aligned");
  SwdStatP p;
  p.x = desc; p.out = out; p.n = n;
  p.blocks = (n + SWD_STAT_ROWS - 1) / SWD_STAT_ROWS;
  p.sum = (double*)ws;
  p.sq = p.sum + 3 * SWD_MAX_STAT_BLOCKS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_swd_sum<0>, dim3(p.blocks), dim3(SWD_STAT_THREADS), 0, st, p);
  hipLaunchKernelGGL(k_swd_sum<1>, dim3(p.blocks), dim3(SWD_STAT_THREADS), 0, st, p);
  hipLaunchKernelGGL(k_swd_norm, dim3(p.blocks), dim3(SWD_STAT_THREADS), 0, st, p);
  VCG_LAUNCH_CHECK("vcg_swd_normalize");
  return 0;
}

// ---- projection --------------------------------------------------------------------------------------------------------------------

#define SP_TM 64
#define SP_TN 64
#define SP_TK 32
#define SP_LD 65                  // row pitch of an LDS tile [k][64] (freq_loss.hip, FF_LD)

struct SwdProjP {
  const float* desc;     // (n, K)
  const float* dirs;     // (K, ndir)
  float* out;            // (ndir, n)
  int n, K, ndir;
};

__global__ __launch_bounds__(256) void k_swd_project(SwdProjP p) {
  __shared__ float sA[SP_TK * SP_LD];                        // A[k][i] = dirs[k][m0 + i]
  __shared__ float sB[SP_TK * SP_LD];                        // B[k][j] = desc[n0 + j][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * SP_TM, n0 = blockIdx.x * SP_TN;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  for (int k0 = 0; k0 < p.K; k0 += SP_TK) {
    __syncthreads();                                         // the last chunk's reads are done
    for (int e = tid; e < SP_TM * SP_TK; e += 256) {         // i fastest: along the rows of dirs
      const int i = e & (SP_TM - 1), kk = e >> 6, m = m0 + i, k = k0 + kk;
      sA[kk * SP_LD + i] = (m < p.ndir && k < p.K) ? p.dirs[(size_t)k * p.ndir + m] : 0.f;
    }
    for (int e = tid; e < SP_TN * SP_TK; e += 256) {         // k fastest: along the rows of desc
      const int kk = e & (SP_TK - 1), j = e >> 5, r = n0 + j, k = k0 + kk;
      sB[kk * SP_LD + j] = (r < p.n && k < p.K) ? p.desc[(size_t)r * p.K + k] : 0.f;
    }
    __syncthreads();
    // lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31] of a 32 x 32 x 2 step
#pragma unroll 4
    for (int kk = 0; kk < SP_TK; kk += 2) {
      const int k = kk + (lane >> 5);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[k * SP_LD + wm * 32 + (lane & 31)], sB[k * SP_LD + wn * 32 + (lane & 31)], acc,
                                                 0, 0, 0);
    }
  }
  // C: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = n0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = m0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
    if (row < p.ndir && col < p.n) p.out[(size_t)row * p.n + col] = acc[q];
  }
}

extern "C" int vcg_swd_project(const float* desc, const float* dirs, float* out, int n, int K, int ndir, void* stream) {
  VCG_CHECK_ARG(desc && dirs && out, "vcg_swd_project: null pointer");
  if (swd_rows_ok("vcg_swd_project", n) != 0) return -1;
  VCG_CHECK_ARG(K >= 1 && K <= 65536 && ndir >= 1 && ndir <= 65535 * SP_TM, "vcg_swd_project: bad K=%d ndir=%d", K, ndir);
  VCG_CHECK_ARG((((uintptr_t)desc | (uintptr_t)dirs | (uintptr_t)out) & 3) == 0, "vcg_swd_project: matrices not 4-byte aligned");
  SwdProjP p;
  p.desc = desc; p.dirs = dirs; p.out = out; p.n = n; p.K = K; p.ndir = ndir;
  const dim3 grid((n + SP_TN - 1) / SP_TN, (ndir + SP_TM - 1) / SP_TM);
  hipLaunchKernelGGL(k_swd_project, grid, dim3(256), 0, (hipStream_t)stream, p);
  VCG_LAUNCH_CHECK("vcg_swd_project");
  return 0;
}

// ---- column sort -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SWD_SORT_THREADS) void k_sort_columns(const float* x, float* out, int n, int P, size_t rs, size_t cs) {
  extern __shared__ float key[];                             // P keys
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * cs;
  for (int i = tid; i < P; i += SWD_SORT_THREADS) key[i] = i < n ? x[base + (size_t)i * rs] : INFINITY;
  __syncthreads();
  const int half = P >> 1;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < half; t += SWD_SORT_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;      // i < l < P
        const float a = key[i], b = key[l];
        const bool swap = (i & k) == 0 ? a > b : a < b;
        if (swap) { key[i] = b; key[l] = a; }
      }
      __syncthreads();
    }
  for (int i = tid; i < n; i += SWD_SORT_THREADS) out[base + (size_t)i * rs] = key[i];
}

extern "C" int vcg_sort_columns(const float* x, float* out, int n, int cols, size_t row_stride, size_t col_stride, void* stream) {
  VCG_CHECK_ARG(x && out, "vcg_sort_columns: null pointer");
  VCG_CHECK_ARG(n >= 1 && n <= VCG_SWD_MAX_DESC, "vcg_sort_columns: %d rows (1 .. %d: a column is sorted in 64 KiB of LDS)", n,
                VCG_SWD_MAX_DESC);
  VCG_CHECK_ARG(cols >= 1, "vcg_sort_columns: bad cols=%d", cols);
  VCG_CHECK_ARG((row_stride == 1 && col_stride >= (size_t)n) || (col_stride == 1 && row_stride >= (size_t)cols),
                "vcg_sort_columns: strides (%zu, %zu) do not describe a dense %d x %d matrix", row_stride, col_stride, n, cols);
  VCG_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "vcg_sort_columns: matrices not 4-byte aligned");
  int P = 1;
  while (P < n) P <<= 1;
  hipLaunchKernelGGL(k_sort_columns, dim3(cols), dim3(SWD_SORT_THREADS), (size_t)P * sizeof(float), (hipStream_t)stream, x, out, n,
                     P, row_stride, col_stride);
  VCG_LAUNCH_CHECK("vcg_sort_columns");
  return 0;
}

// ---- distance ----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_swd_dist(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ slots,
                                                  size_t n, size_t chunk) {
  __shared__ double red[256 / VCG_WAVE];
  const int tid = threadIdx.x;
  const size_t i0 = (size_t)blockIdx.x * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
  double s = 0.0;
  for (size_t i = i0 + tid; i < i1; i += 256) s += fabs((double)a[i] - (double)b[i]);
  s = wave_sum_d(s);
  if ((tid & (VCG_WAVE - 1)) == 0) red[tid / VCG_WAVE] = s;
  __syncthreads();
  if (tid == 0) slots[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_swd_dist_final(const double* __restrict__ slots, int blocks, double inv_count,
                                                        float* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < blocks; i += 256) s += slots[i];
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[0] = (float)(red[0] * inv_count);
}

// chunk: SWD_DIST_CHUNK elements per workgroup, more where that would pass SWD_DIST_MAX_BLOCKS slots
static size_t swd_dist_chunk(size_t n) {
  size_t chunk = SWD_DIST_CHUNK;
  while ((n + chunk - 1) / chunk > SWD_DIST_MAX_BLOCKS) chunk *= 2;
  return chunk;
}

extern "C" size_t vcg_swd_distance_workspace(size_t n) {
  if (n == 0) {
    vcg_set_error("vcg_swd_distance_workspace: n == 0");
    return 0;
  }
  const size_t chunk = swd_dist_chunk(n);
  return ((n + chunk - 1) / chunk * sizeof(double) + 15) / 16 * 16;
}

extern "C" int vcg_swd_distance(const float* a, const float* b, float* out, size_t n, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(a && b && out && ws, "vcg_swd_distance: null pointer");
  VCG_CHECK_ARG(n > 0, "vcg_swd_distance: n == 0");
  VCG_CHECK_ARG(ws_bytes >= vcg_swd_distance_workspace(n), "vcg_swd_distance: workspace of %zu bytes, %zu needed", ws_bytes,
                vcg_swd_distance_workspace(n));
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_swd_distance: workspace not 16-byte aligned");
  VCG_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3) == 0, "vcg_swd_distance: pointers not 4-byte aligned");
  const size_t chunk = swd_dist_chunk(n);
  const int blocks = (int)((n + chunk - 1) / chunk);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_swd_dist, dim3(blocks), dim3(256), 0, st, a, b, (double*)ws, n, chunk);
  hipLaunchKernelGGL(k_swd_dist_final, dim3(1), dim3(256), 0, st, (const double*)ws, blocks, 1.0 / (double)n, out);
  VCG_LAUNCH_CHECK("vcg_swd_distance");
  return 0;
}
