// Sliced Wasserstein distance as a TRAINING loss between the set {G(x)} and the set {y}: what swd.hip's evaluator score lacks for
// a gradient.  DESIGN.md, "Sliced Wasserstein training loss", has the definition.  A level of the loss goes through
//
// k_swd_pool          level k + 1 = the 2 x 2 mean of level k on (N, H, W, 4): a plain box pyramid (not the evaluator's Laplacian
//                     one), because its adjoint is a 1/4 spread.  The four values are added in double and rounded once.
// k_swd_grid_gather   the level is cut into s x s cells; every cell gives the one 7 x 7 x 3 patch at the in-cell offset (oy, ox),
//                     flattened (c, dy, dx) as k_swd_gather does.  (s, oy, ox) travel by value: no plan array, no host memory.
// (k_swd_project)     swd.hip's projection, unchanged, forward AND backward: gdesc = gproj^T dirs^T is the same contraction with
//                     desc := dirs (147 rows of K = 128) and dirs := gproj (128, n).
// k_sort_columns_indexed  bitonic sort of (key, source row) pairs of one column per workgroup in LDS, ordered by (key, row): the
//                     result of a stable argsort whatever the network's shape.  8192 pairs are the 64 KiB a workgroup may ask
//                     for by default.  Every loop bound depends on n alone.  A column that holds a NaN is left as it came (its
//                     rows 0 .. n - 1 in order): the index half is a permutation of 0 .. n - 1 in every case.
// k_swd_pair          one pass over sorted a and sorted b: |a - b| into double block slots, sign(a - b) through perm_a into
//                     gproj (D, n), unscaled; k_swd_pair_final adds the slots in a fixed order into the running total.
// k_swd_grid_scatter  the adjoint of the gather in gather form: one thread per pixel decides from (s, oy, ox) whether it lies in
//                     a patch, reads its gdesc element per channel or writes 0.  The patches never overlap: no atomics, no order.
// k_swd_pool_adjoint_add  fine += coarse / 4.
// k_swd_unit_columns  every column of a (K, D) matrix scaled to unit 2-norm, the sum in double: the directions of a step, from
//                     vcg_randn's Gaussians, without a host round trip.
// No float atomics anywhere: the same input gives the same bits.
#include <math.h>

#include "vcg_common.h"

#define SL_PATCH 7
#define SL_DESC (3 * SL_PATCH * SL_PATCH)      // 147
#define SL_MIN_CELL 8
#define SL_MIN_SIDE 16
#define SL_GATHER_THREADS 192
#define SL_SORT_THREADS 512
#define SL_PAIR_CHUNK 2048
#define SL_MAX_DIRS 1024
#define SL_MAX_SIDE 32768
#define SL_MAX_PIXELS ((size_t)1 << 38)     // one thread per pixel, 256 per workgroup: under 2^31 workgroups

// ---- shared argument checks ----------------------------------------------------------------------------------------------------------

static int sl_rows_ok(const char* who, int n) {
  VCG_CHECK_ARG(n >= 1 && n <= VCG_SWD_LOSS_MAX_DESC, "%s: %d descriptors (1 .. %d)", who, n, VCG_SWD_LOSS_MAX_DESC);
  return 0;
}

// the cells of an (N, H, W) level and the patch offset inside them
static int sl_grid_ok(const char* who, int N, int H, int W, int s, int oy, int ox) {
  VCG_CHECK_ARG(N >= 1 && N <= 65535, "%s: bad N=%d", who, N);
  VCG_CHECK_ARG(H >= SL_MIN_SIDE && W >= SL_MIN_SIDE && H <= SL_MAX_SIDE && W <= SL_MAX_SIDE,
                "%s: a level of %dx%d (sides %d .. %d)", who, H, W, SL_MIN_SIDE, SL_MAX_SIDE);
  VCG_CHECK_ARG(s >= SL_MIN_CELL && s <= H && s <= W, "%s: cell side %d (%d .. min(H, W) = %d)", who, s, SL_MIN_CELL, H < W ? H : W);
  VCG_CHECK_ARG(oy >= 0 && oy <= s - SL_PATCH && ox >= 0 && ox <= s - SL_PATCH,
                "%s: patch offset (%d, %d) outside [0, %d] of a %dx%d cell", who, oy, ox, s - SL_PATCH, s, s);
  const long long n = (long long)N * (H / s) * (W / s);
  VCG_CHECK_ARG(n >= 1 && n <= VCG_SWD_LOSS_MAX_DESC, "%s: %lld descriptors (1 .. %d)", who, n, VCG_SWD_LOSS_MAX_DESC);
  VCG_CHECK_ARG((size_t)N * H * W <= SL_MAX_PIXELS, "%s: %d images of %dx%d exceed %zu pixels", who, N, H, W, (size_t)SL_MAX_PIXELS);
  return 0;
}

extern "C" int vcg_swd_cell_side(int N, int H, int W) {
  if (N < 1 || H < SL_MIN_SIDE || W < SL_MIN_SIDE || H > SL_MAX_SIDE || W > SL_MAX_SIDE) {
    vcg_set_error("vcg_swd_cell_side: bad N=%d H=%d W=%d (sides %d .. %d)", N, H, W, SL_MIN_SIDE, SL_MAX_SIDE);
    return 0;
  }
  const int lim = H < W ? H : W;
  for (int s = SL_MIN_CELL; s <= lim; ++s)
    if ((long long)N * (H / s) * (W / s) <= VCG_SWD_LOSS_MAX_DESC) return s;
  vcg_set_error("vcg_swd_cell_side: %d images of %dx%d give more than %d descriptors at every cell side", N, H, W,
                VCG_SWD_LOSS_MAX_DESC);
  return 0;
}

extern "C" int vcg_swd_loss_levels(int H, int W) {
  if (H < SL_MIN_SIDE || W < SL_MIN_SIDE || H > SL_MAX_SIDE || W > SL_MAX_SIDE) {
    vcg_set_error("vcg_swd_loss_levels: bad H=%d W=%d (sides %d .. %d)", H, W, SL_MIN_SIDE, SL_MAX_SIDE);
    return 0;
  }
  int levels = 1;
  while (levels < VCG_SWD_LOSS_MAX_LEVELS && H % 2 == 0 && W % 2 == 0 && H / 2 >= SL_MIN_SIDE && W / 2 >= SL_MIN_SIDE) {
    H /= 2; W /= 2; ++levels;
  }
  return levels;
}

// ---- box pyramid ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_swd_pool(const float4* __restrict__ x, float4* __restrict__ out, int N, int Ho, int Wo) {
  const size_t total = (size_t)N * Ho * Wo;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int xo = (int)(i % Wo);
  const size_t row = i / Wo;                                 // n * Ho + yo: the fine rows 2 row, 2 row + 1 (H = 2 Ho)
  const size_t W = 2 * (size_t)Wo;
  const float4* p = x + 2 * row * W + 2 * xo;
  const float4 a = p[0], b = p[1], c = p[W], d = p[W + 1];
  float4 o;
  o.x = (float)((((double)a.x + (double)b.x) + ((double)c.x + (double)d.x)) * 0.25);
  o.y = (float)((((double)a.y + (double)b.y) + ((double)c.y + (double)d.y)) * 0.25);
  o.z = (float)((((double)a.z + (double)b.z) + ((double)c.z + (double)d.z)) * 0.25);
  o.w = 0.f;
  out[i] = o;
}

__global__ __launch_bounds__(256) void k_swd_pool_adjoint_add(const float4* __restrict__ coarse, float4* __restrict__ fine, int N, int H,
                                                              int W) {
  const size_t total = (size_t)N * H * W;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % W);
  const size_t row = i / W;
  const int y = (int)(row % H);
  const size_t n = row / H;
  const float4 c = coarse[(n * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1)];
  float4 f = fine[i];
  f.x = fmaf(0.25f, c.x, f.x); f.y = fmaf(0.25f, c.y, f.y); f.z = fmaf(0.25f, c.z, f.z);
  fine[i] = f;
}

static int sl_pool_ok(const char* who, const void* fine, const void* coarse, int N, int H, int W) {
  VCG_CHECK_ARG(fine && coarse, "%s: null pointer", who);
  VCG_CHECK_ARG(N >= 1 && N <= 65535, "%s: bad N=%d", who, N);
  VCG_CHECK_ARG(H % 2 == 0 && W % 2 == 0 && H / 2 >= SL_MIN_SIDE && W / 2 >= SL_MIN_SIDE && H <= SL_MAX_SIDE && W <= SL_MAX_SIDE,
                "%s: a %dx%d level has no coarser one (even sides, halves of at least %d)", who, H, W, SL_MIN_SIDE);
  VCG_CHECK_ARG((((uintptr_t)fine | (uintptr_t)coarse) & 15) == 0, "%s: images not 16-byte aligned", who);
  VCG_CHECK_ARG(fine != coarse, "%s: the buffers must be distinct", who);
  VCG_CHECK_ARG((size_t)N * H * W <= SL_MAX_PIXELS, "%s: %d images of %dx%d exceed %zu pixels", who, N, H, W, (size_t)SL_MAX_PIXELS);
  return 0;
}

extern "C" int vcg_swd_pool(const float* x, float* out, int N, int H, int W, void* stream) {
  if (sl_pool_ok("vcg_swd_pool", x, out, N, H, W) != 0) return -1;
  const size_t total = (size_t)N * (H / 2) * (W / 2);
  hipLaunchKernelGGL(k_swd_pool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)x, (float4*)out,
                     N, H / 2, W / 2);
  VCG_LAUNCH_CHECK("vcg_swd_pool");
  return 0;
}

extern "C" int vcg_swd_pool_adjoint_add(const float* coarse, float* fine, int N, int H, int W, void* stream) {
  if (sl_pool_ok("vcg_swd_pool_adjoint_add", fine, coarse, N, H, W) != 0) return -1;
  const size_t total = (size_t)N * H * W;
  hipLaunchKernelGGL(k_swd_pool_adjoint_add, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)coarse, (float4*)fine, N, H, W);
  VCG_LAUNCH_CHECK("vcg_swd_pool_adjoint_add");
  return 0;
}

// ---- descriptors on a grid of cells ------------------------------------------------------------------------------------------------

struct SwdGridP {
  int H, W, s, oy, ox, cy, cx;      // cy = H / s, cx = W / s cells per image
};

__global__ __launch_bounds__(SL_GATHER_THREADS) void k_swd_grid_gather(SwdGridP g, const float* __restrict__ lvl, float* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= SL_DESC) return;
  const int d = blockIdx.x, c = t / 49, rem = t - 49 * c, dy = rem / 7, dx = rem - 7 * dy;
  const int cell = d % (g.cy * g.cx), n = d / (g.cy * g.cx), ci = cell / g.cx, cj = cell - ci * g.cx;
  const int y = ci * g.s + g.oy + dy, x = cj * g.s + g.ox + dx;      // < cy s <= H, < cx s <= W
  out[(size_t)d * SL_DESC + t] = lvl[(((size_t)n * g.H + y) * g.W + x) * 4 + c];
}

// mul = scale * (*gscale, or 1): the backward's g / (n D levels)
__global__ __launch_bounds__(256) void k_swd_grid_scatter(SwdGridP g, const float* __restrict__ gdesc, const float* __restrict__ gscale,
                                                          float scale, float4* __restrict__ out, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % g.W);
  const size_t row = i / g.W;
  const int y = (int)(row % g.H), n = (int)(row / g.H);
  const int ci = y / g.s, cj = x / g.s, dy = y - ci * g.s - g.oy, dx = x - cj * g.s - g.ox;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ci < g.cy && cj < g.cx && dy >= 0 && dy < SL_PATCH && dx >= 0 && dx < SL_PATCH) {
    const float mul = gscale ? scale * gscale[0] : scale;
    const float* p = gdesc + ((size_t)(n * g.cy + ci) * g.cx + cj) * SL_DESC + dy * 7 + dx;
    o.x = p[0] * mul; o.y = p[49] * mul; o.z = p[98] * mul;
  }
  out[i] = o;
}

static SwdGridP sl_grid(int H, int W, int s, int oy, int ox) {
  SwdGridP g;
  g.H = H; g.W = W; g.s = s; g.oy = oy; g.ox = ox; g.cy = H / s; g.cx = W / s;
  return g;
}

extern "C" int vcg_swd_grid_gather(const float* level, float* out, int N, int H, int W, int s, int oy, int ox, void* stream) {
  VCG_CHECK_ARG(level && out, "vcg_swd_grid_gather: null pointer");
  if (sl_grid_ok("vcg_swd_grid_gather", N, H, W, s, oy, ox) != 0) return -1;
  VCG_CHECK_ARG((((uintptr_t)level | (uintptr_t)out) & 3) == 0, "vcg_swd_grid_gather: pointers not 4-byte aligned");
  const SwdGridP g = sl_grid(H, W, s, oy, ox);
  hipLaunchKernelGGL(k_swd_grid_gather, dim3(N * g.cy * g.cx), dim3(SL_GATHER_THREADS), 0, (hipStream_t)stream, g, level, out);
  VCG_LAUNCH_CHECK("vcg_swd_grid_gather");
  return 0;
}

extern "C" int vcg_swd_grid_scatter(const float* gdesc, const float* gscale, float scale, float* out, int N, int H, int W, int s, int oy,
                                    int ox, void* stream) {
  VCG_CHECK_ARG(gdesc && out, "vcg_swd_grid_scatter: null pointer");
  if (sl_grid_ok("vcg_swd_grid_scatter", N, H, W, s, oy, ox) != 0) return -1;
  VCG_CHECK_ARG(isfinite(scale), "vcg_swd_grid_scatter: scale is not finite");
  VCG_CHECK_ARG((((uintptr_t)gdesc | (uintptr_t)gscale) & 3) == 0 && ((uintptr_t)out & 15) == 0,
                "vcg_swd_grid_scatter: gdesc / gscale not 4-byte or out not 16-byte aligned");
  const SwdGridP g = sl_grid(H, W, s, oy, ox);
  const size_t total = (size_t)N * H * W;
  hipLaunchKernelGGL(k_swd_grid_scatter, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, gdesc, gscale, scale,
                     (float4*)out, total);
  VCG_LAUNCH_CHECK("vcg_swd_grid_scatter");
  return 0;
}

// ---- indexed column sort ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SL_SORT_THREADS) void k_sort_columns_indexed(const float* x, float* keys, int32_t* rows, int n, int P,
                                                                           size_t rs, size_t cs) {
  extern __shared__ float sl_lds[];                          // P keys, then P source rows
  float* key = sl_lds;
  int32_t* idx = (int32_t*)(sl_lds + P);
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * cs;
  int bad = 0;
  for (int i = tid; i < P; i += SL_SORT_THREADS) {
    const float v = i < n ? x[base + (size_t)i * rs] : INFINITY;
    bad |= v != v;
    key[i] = v;
    idx[i] = i;                                              // the pads (+inf, n ..) follow every real (+inf, row < n)
  }
  // a NaN compares false both ways: a network that kept exchanging the other keys around it could leave a pad among the first
  // n pairs.  Such a column exchanges nothing (same loops, same barriers) and comes out as it came
  const bool live = __syncthreads_or(bad) == 0;
  const int half = P >> 1;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < half; t += SL_SORT_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;      // i < l < P
        const float a = key[i], b = key[l];
        const int ia = idx[i], ib = idx[l];
        const bool gt = a > b || (a == b && ia > ib), lt = a < b || (a == b && ia < ib);
        if (live && ((i & k) == 0 ? gt : lt)) { key[i] = b; key[l] = a; idx[i] = ib; idx[l] = ia; }
      }
      __syncthreads();
    }
  for (int i = tid; i < n; i += SL_SORT_THREADS) {
    keys[base + (size_t)i * rs] = key[i];
    rows[base + (size_t)i * rs] = idx[i];
  }
}

extern "C" int vcg_sort_columns_indexed(const float* x, float* keys, int32_t* rows, int n, int cols, size_t row_stride,
                                        size_t col_stride, void* stream) {
  VCG_CHECK_ARG(x && keys && rows, "vcg_sort_columns_indexed: null pointer");
  VCG_CHECK_ARG(n >= 1 && n <= VCG_SWD_LOSS_MAX_DESC, "vcg_sort_columns_indexed: %d rows (1 .. %d: a column's keys and rows are sorted in 64 KiB of LDS)",
                n, VCG_SWD_LOSS_MAX_DESC);
  VCG_CHECK_ARG(cols >= 1, "vcg_sort_columns_indexed: bad cols=%d", cols);
  VCG_CHECK_ARG((row_stride == 1 && col_stride >= (size_t)n) || (col_stride == 1 && row_stride >= (size_t)cols),
                "vcg_sort_columns_indexed: strides (%zu, %zu) do not describe a dense %d x %d matrix", row_stride, col_stride, n, cols);
  VCG_CHECK_ARG((((uintptr_t)x | (uintptr_t)keys | (uintptr_t)rows) & 3) == 0, "vcg_sort_columns_indexed: matrices not 4-byte aligned");
  VCG_CHECK_ARG((const void*)keys != (const void*)rows, "vcg_sort_columns_indexed: keys and rows must be distinct");
  int P = 1;
  while (P < n) P <<= 1;
  hipLaunchKernelGGL(k_sort_columns_indexed, dim3(cols), dim3(SL_SORT_THREADS), (size_t)P * (sizeof(float) + sizeof(int32_t)),
                     (hipStream_t)stream, x, keys, rows, n, P, row_stride, col_stride);
  VCG_LAUNCH_CHECK("vcg_sort_columns_indexed");
  return 0;
}

// ---- the sorted pairing: value and signed gradient --------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_swd_pair(const float* __restrict__ a, const float* __restrict__ b, const int32_t* __restrict__ perm,
                                                  float* __restrict__ gproj, double* __restrict__ slots, int n, size_t total) {
  __shared__ double red[256 / VCG_WAVE];
  const int tid = threadIdx.x;
  const size_t i0 = (size_t)blockIdx.x * SL_PAIR_CHUNK, i1 = i0 + SL_PAIR_CHUNK < total ? i0 + SL_PAIR_CHUNK : total;
  double s = 0.0;
  for (size_t i = i0 + tid; i < i1; i += 256) {
    const float va = a[i], vb = b[i];
    s += fabs((double)va - (double)vb);
    const size_t col = i / (size_t)n;
    const int32_t p = perm[i];                               // a permutation of 0 .. n - 1 per column; anything else is skipped
    if ((uint32_t)p < (uint32_t)n) gproj[col * n + p] = va > vb ? 1.f : (va < vb ? -1.f : 0.f);      // a NaN: 0
  }
  s = wave_sum_d(s);
  if ((tid & (VCG_WAVE - 1)) == 0) red[tid / VCG_WAVE] = s;
  __syncthreads();
  if (tid == 0) slots[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// total = (accumulate ? total : 0) + weight * sum(slots) / count; out = (float)total
__global__ __launch_bounds__(256) void k_swd_pair_final(const double* __restrict__ slots, int blocks, double weight_over_count, int accumulate,
                                                        double* __restrict__ total, float* __restrict__ out) {
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
  if (tid == 0) {
    const double t = (accumulate ? total[0] : 0.0) + red[0] * weight_over_count;
    total[0] = t;
    out[0] = (float)t;
  }
}

static int sl_pair_ok(const char* who, int n, int ndir) {
  if (sl_rows_ok(who, n) != 0) return -1;
  VCG_CHECK_ARG(ndir >= 1 && ndir <= SL_MAX_DIRS, "%s: %d directions (1 .. %d)", who, ndir, SL_MAX_DIRS);
  return 0;
}

extern "C" size_t vcg_swd_pair_loss_workspace(int n, int ndir) {
  if (sl_pair_ok("vcg_swd_pair_loss_workspace", n, ndir) != 0) return 0;
  const size_t total = (size_t)n * ndir;
  return ((total + SL_PAIR_CHUNK - 1) / SL_PAIR_CHUNK * sizeof(double) + 15) / 16 * 16;
}

extern "C" int vcg_swd_pair_loss(const float* a_sorted, const float* b_sorted, const int32_t* perm_a, float* gproj, int n, int ndir,
                                 double weight, int accumulate, double* total, float* out, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(a_sorted && b_sorted && perm_a && gproj && total && out && ws, "vcg_swd_pair_loss: null pointer");
  if (sl_pair_ok("vcg_swd_pair_loss", n, ndir) != 0) return -1;
  VCG_CHECK_ARG(isfinite(weight), "vcg_swd_pair_loss: weight is not finite");
  VCG_CHECK_ARG(ws_bytes >= vcg_swd_pair_loss_workspace(n, ndir), "vcg_swd_pair_loss: workspace of %zu bytes, %zu needed", ws_bytes,
                vcg_swd_pair_loss_workspace(n, ndir));
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)total & 7) == 0, "vcg_swd_pair_loss: workspace not 16-byte or total not 8-byte aligned");
  VCG_CHECK_ARG((((uintptr_t)a_sorted | (uintptr_t)b_sorted | (uintptr_t)perm_a | (uintptr_t)gproj | (uintptr_t)out) & 3) == 0,
                "vcg_swd_pair_loss: pointers not 4-byte aligned");
  VCG_CHECK_ARG(gproj != a_sorted && gproj != b_sorted && (const void*)gproj != (const void*)perm_a,
                "vcg_swd_pair_loss: gproj must not alias an input");
  const size_t count = (size_t)n * ndir;
  const int blocks = (int)((count + SL_PAIR_CHUNK - 1) / SL_PAIR_CHUNK);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_swd_pair, dim3(blocks), dim3(256), 0, st, a_sorted, b_sorted, perm_a, gproj, (double*)ws, n, count);
  hipLaunchKernelGGL(k_swd_pair_final, dim3(1), dim3(256), 0, st, (const double*)ws, blocks, weight / (double)count, accumulate != 0, total,
                     out);
  VCG_LAUNCH_CHECK("vcg_swd_pair_loss");
  return 0;
}

// ---- unit directions ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(VCG_WAVE) void k_swd_unit_columns(const float* __restrict__ x, float* __restrict__ out, int K, int D) {
  const int j = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int k = lane; k < K; k += VCG_WAVE) {
    const double v = (double)x[(size_t)k * D + j];
    s += v * v;
  }
  s = wave_sum_d(s);                                          // every lane holds the same sum
  const double inv = 1.0 / sqrt(s);                          // a zero column comes out NaN
  for (int k = lane; k < K; k += VCG_WAVE) out[(size_t)k * D + j] = (float)((double)x[(size_t)k * D + j] * inv);
}

extern "C" int vcg_swd_unit_columns(const float* x, float* out, int K, int D, void* stream) {
  VCG_CHECK_ARG(x && out, "vcg_swd_unit_columns: null pointer");
  VCG_CHECK_ARG(K >= 1 && K <= 65536 && D >= 1 && D <= 65535, "vcg_swd_unit_columns: bad K=%d D=%d", K, D);
  VCG_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "vcg_swd_unit_columns: matrices not 4-byte aligned");
  hipLaunchKernelGGL(k_swd_unit_columns, dim3(D), dim3(VCG_WAVE), 0, (hipStream_t)stream, x, out, K, D);
  VCG_LAUNCH_CHECK("vcg_swd_unit_columns");
  return 0;
}
