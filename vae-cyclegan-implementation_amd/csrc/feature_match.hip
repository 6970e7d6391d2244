// Discriminator feature-matching loss (new: the reference has no such term).  The generator is asked to reproduce the discriminator's
// intermediate activations on real images: f_l, r_l are the outputs of up to VCG_FM_MAX_LAYERS blocks on the generated and on the
// real batch.  Kernels of their own: a run with the weight at its default 0 launches nothing from this file.
//
//   f_l, r_l: R_l x Cp_l fp32, the networks' NHWC buffers with R_l = N h w rows, C_l logical channels at pitch Cp_l = 4 ceil(C_l / 4),
//   the channel the fastest index.  Pad lanes hold zeros in both operands.  With L layers and k_l = 1 / (L R_l C_l):
//
//     pair   fm = sum_l k_l sum_e |f_l[e] - r_l[e]|                         (pix2pixHD: image i of one batch belongs to image i of the other)
//     mean   fm = sum_l k_l R_l sum_c |D_lc|,  D_lc = (1 / R_l) sum_rows (f_l - r_l)[row, c]    (Salimans et al. 2016: match the expected features)
//
//   The real side is a constant of the term.  d fm / d f_l[e] = k_l sign(f_l[e] - r_l[e]) (pair), k_l sign(D_lc) (mean), sign(0) = 0.
//
//   forward, two launches (pair) or three (mean), all layers in each:
//     pair   k_fm_pair_partial  every layer is cut into chunks of FM_PAIR_CHUNK float4s; the chunks of all layers form one flat space that
//                               at most FM_MAX_BLOCKS workgroups stride over.  A lane sums |f - r| of its float4s of a chunk in double,
//                               weighs the chunk's sum with k_l, and the workgroup's lanes are combined by a butterfly of shuffles and
//                               through LDS in wavefront order: one double per workgroup.
//            k_fm_final         one workgroup sums them in a fixed order and rounds ONCE to fp32.
//     mean   k_fm_mean_partial  a workgroup owns a slab of rows x a group of channel quads of one layer: lane (r, q) reads quad q of its rows
//                               (lanes of one row are neighbours along the channel: coalesced) and sums f - r per channel in double; the
//                               row lanes are combined through LDS in a fixed tree.  One double per (slab, channel).
//            k_fm_mean_channels one workgroup per (layer, 64 channels): per channel the slabs are summed in a fixed order, D_lc formed in
//                               double, sign(D_lc) stored (one float per channel of the pitch and layer, 0 in the pad lanes) and the group's
//                               k_l R_l |D_lc| summed in a fixed order: one double per workgroup.  (One workgroup for all channels would
//                               read the two MB of partials of a batch of 8 by itself, longer than the pass over the activations takes.)
//            k_fm_final         sums the groups in a fixed order; one rounding to fp32.
//   backward, one launch over the chunks of all layers: c_l = (float)((double)g k_l), and every element gets +c_l, -c_l or 0 — by the sign
//   recomputed from f_l, r_l (pair) or the stored channel sign (mean).  Pad lanes of the gradient are written as zeros.
//
// No atomics; every sum has a fixed order, so the same input gives the same bits.  A NaN in a layer reaches the loss (pair: through its
// summand; mean: through its channel's D_lc) and its own gradient elements.  The layer descriptors travel by value in the kernel
// arguments: no upload, no host synchronisation.  Plain C++, vector loads and stores only.
#include <math.h>

#include "vcg_common.h"

#define FM_THREADS 256
#define FM_WAVES (FM_THREADS / 64)
#define FM_MAX_LAYERS VCG_FM_MAX_LAYERS
#define FM_PAIR_CHUNK 2048      // float4s of one layer per chunk: 8 per lane, 32 KiB of each operand
#define FM_MAX_BLOCKS 2048      // workgroups of the chunk-strided launches (pair forward, backward)
#define FM_MAX_TC 64            // channel quads per workgroup of the mean kernel (256 channels); the other lanes are row lanes
#define FM_MEAN_RPL 16          // rows per row lane of a slab
#define FM_FINAL_THREADS 1024
#define FM_FINAL_CW 64          // the mean channel pass: 64 channels x 16 slab lanes per workgroup
#define FM_FINAL_RL (FM_FINAL_THREADS / FM_FINAL_CW)

enum { FM_PAIR = VCG_FM_PAIR, FM_MEAN = VCG_FM_MEAN };

struct FmLayer {
  const float* f;               // generated side; real side (null in the mean backward: the signs stand for both)
  const float* r;
  float* g;                     // backward: the layer's gradient buffer, null when it needs none
  size_t rows, n4;              // n4 = rows cp4 float4s
  size_t first;                 // index of the layer's first chunk (pair, backward) or workgroup (mean) in the flat space
  size_t part;                  // mean: offset of the layer's partials [nslab][cp] in the workspace, in doubles
  size_t slab, nslab;           // mean: rows per workgroup, workgroups along the rows
  double k;                     // 1 / (L rows c)
  int c, cp4;                   // logical channels, float4s per row
  int tc, tc_log2, cgroups;     // mean: quad lanes of a workgroup (a power of two), workgroups along the channel
  int sign0;                    // mean: offset of the layer's channel signs [cp]: a multiple of 4
  int group0;                   // mean: index of the layer's first group of FM_FINAL_CW channels
};

struct FmPlan {
  FmLayer l[FM_MAX_LAYERS];
  int n;
  size_t total;                 // chunks (pair, backward) or workgroups (mean) of all layers
  int groups;                   // mean: channel groups of all layers
};

// sign(d) k with sign(0) = 0; a NaN stays one
__device__ __forceinline__ float fm_signed(float d, float k) { return d > 0.f ? k : (d < 0.f ? -k : (d != d ? d : 0.f)); }

// the layer whose range of the flat space holds index i (layers are in ascending order of `first`)
__device__ __forceinline__ int fm_layer_of(const FmPlan& p, size_t i) {
  int l = 0;
#pragma unroll
  for (int j = 1; j < FM_MAX_LAYERS; ++j)
    if (j < p.n && i >= p.l[j].first) l = j;
  return l;
}

// combines the workgroup's doubles in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double fm_block_sum(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < FM_WAVES; ++w) s += red[w];
  return s;
}

// ------------------------------------------------------------------------------------------------------------------ pair
__global__ __launch_bounds__(FM_THREADS) void k_fm_pair_partial(FmPlan p, double* __restrict__ part) {
  __shared__ double red[FM_WAVES];
  double acc = 0.0;
  for (size_t ch = blockIdx.x; ch < p.total; ch += gridDim.x) {
    const int li = fm_layer_of(p, ch);
    const FmLayer& L = p.l[li];
    const size_t q0 = (ch - L.first) * FM_PAIR_CHUNK;
    const size_t q1 = q0 + FM_PAIR_CHUNK < L.n4 ? q0 + FM_PAIR_CHUNK : L.n4;
    const float4* __restrict__ f4 = reinterpret_cast<const float4*>(L.f);
    const float4* __restrict__ r4 = reinterpret_cast<const float4*>(L.r);
    double s = 0.0;
#pragma unroll 4
    for (size_t q = q0 + threadIdx.x; q < q1; q += FM_THREADS) {
      const float4 a = f4[q], b = r4[q];
      s += fabs((double)a.x - (double)b.x);
      s += fabs((double)a.y - (double)b.y);
      s += fabs((double)a.z - (double)b.z);
      s += fabs((double)a.w - (double)b.w);
    }
    acc += s * L.k;
  }
  const double total = fm_block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(FM_FINAL_THREADS) void k_fm_final(const double* __restrict__ part, int nblocks,
                                                                    float* __restrict__ out) {
  __shared__ double red[FM_FINAL_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += FM_FINAL_THREADS) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = FM_FINAL_THREADS >> 1; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)red[0];
}

// ------------------------------------------------------------------------------------------------------------------ mean
// one workgroup per (layer, slab, channel group): blockIdx.x - first = slab * cgroups + channel group
__global__ __launch_bounds__(FM_THREADS) void k_fm_mean_partial(FmPlan p, double* __restrict__ part) {
  __shared__ double red[4][FM_THREADS];
  const int li = fm_layer_of(p, blockIdx.x);
  const FmLayer& L = p.l[li];
  const size_t wg = blockIdx.x - L.first;
  const size_t slab = wg / (size_t)L.cgroups;
  const int cg = (int)(wg - slab * (size_t)L.cgroups);
  const int tid = threadIdx.x, q = tid & (L.tc - 1), r = tid >> L.tc_log2, tp = FM_THREADS >> L.tc_log2;
  const int cq = cg * L.tc + q;
  const size_t row0 = slab * L.slab;
  const size_t row1 = row0 + L.slab < L.rows ? row0 + L.slab : L.rows;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (cq < L.cp4) {
    const float4* __restrict__ f4 = reinterpret_cast<const float4*>(L.f);
    const float4* __restrict__ r4 = reinterpret_cast<const float4*>(L.r);
#pragma unroll 4
    for (size_t row = row0 + r; row < row1; row += tp) {
      const float4 a = f4[row * L.cp4 + cq], b = r4[row * L.cp4 + cq];
      s0 += (double)a.x - (double)b.x;
      s1 += (double)a.y - (double)b.y;
      s2 += (double)a.z - (double)b.z;
      s3 += (double)a.w - (double)b.w;
    }
  }
  red[0][tid] = s0;
  red[1][tid] = s1;
  red[2][tid] = s2;
  red[3][tid] = s3;
  __syncthreads();
  for (int h = tp >> 1; h > 0; h >>= 1) {          // row lane r takes row lane r + h: the same tree for every input
    if (r < h) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[j][tid] += red[j][tid + h * L.tc];
    }
    __syncthreads();
  }
  if (r == 0 && cq < L.cp4) {
    double* dst = part + L.part + slab * (size_t)(4 * L.cp4) + 4 * cq;
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = red[j][tid];
  }
}

// One workgroup per (layer, group of FM_FINAL_CW channels), thread (slab lane r, channel lane q): slab lane r sums the slabs r, r + RL,
// r + 2 RL, ... of its channel in that order, the RL lane sums are added in lane order by lane 0, which forms D_lc; the group's
// contributions meet in the first wavefront's butterfly.  gpart [groups].
__global__ __launch_bounds__(FM_FINAL_THREADS) void k_fm_mean_channels(FmPlan p, const double* __restrict__ part,
                                                                       float* __restrict__ signs, double* __restrict__ gpart) {
  __shared__ double red[FM_FINAL_RL][FM_FINAL_CW];
  int li = 0;
#pragma unroll
  for (int j = 1; j < FM_MAX_LAYERS; ++j)
    if (j < p.n && (int)blockIdx.x >= p.l[j].group0) li = j;
  const FmLayer& L = p.l[li];
  const int q = threadIdx.x & (FM_FINAL_CW - 1), r = threadIdx.x / FM_FINAL_CW;
  const int cp = 4 * L.cp4, ch = ((int)blockIdx.x - L.group0) * FM_FINAL_CW + q;
  double s = 0.0;
  if (ch < L.c) {
    const double* src = part + L.part + ch;
    size_t i = r;
    for (; i + 7 * FM_FINAL_RL < L.nslab; i += 8 * FM_FINAL_RL) {           // eight loads in flight, added in slab order
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[(i + j * FM_FINAL_RL) * cp];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; i < L.nslab; i += FM_FINAL_RL) s += src[i * cp];
  }
  red[r][q] = s;
  __syncthreads();
  if (r == 0) {                                    // the first wavefront
    double acc = 0.0;
    if (ch < L.c) {
      double d = red[0][q];
#pragma unroll
      for (int j = 1; j < FM_FINAL_RL; ++j) d += red[j][q];
      d /= (double)L.rows;
      signs[L.sign0 + ch] = d > 0.0 ? 1.f : (d < 0.0 ? -1.f : (d != d ? (float)d : 0.f));      // a NaN stays one
      acc = fabs(d) * (L.k * (double)L.rows);
    } else if (ch < cp) {
      signs[L.sign0 + ch] = 0.f;                   // a pad lane
    }
    acc = wave_sum_d(acc);
    if (threadIdx.x == 0) gpart[blockIdx.x] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// strides over the chunks of the layers that want a gradient
template <int MODE>
__global__ __launch_bounds__(FM_THREADS) void k_fm_bwd(FmPlan p, const float* __restrict__ gout, const float* __restrict__ signs) {
  const double g = (double)gout[0];
  for (size_t ch = blockIdx.x; ch < p.total; ch += gridDim.x) {
    const int li = fm_layer_of(p, ch);
    const FmLayer& L = p.l[li];
    const float k = (float)(g * L.k);              // one rounding
    const size_t q0 = (ch - L.first) * FM_PAIR_CHUNK;
    const size_t q1 = q0 + FM_PAIR_CHUNK < L.n4 ? q0 + FM_PAIR_CHUNK : L.n4;
    const unsigned cp4 = (unsigned)L.cp4, lane0 = (unsigned)(q0 % cp4);
    float4* __restrict__ g4 = reinterpret_cast<float4*>(L.g);
    for (size_t q = q0 + threadIdx.x; q < q1; q += FM_THREADS) {
      const int c0 = 4 * (int)((lane0 + (unsigned)(q - q0)) % cp4);
      float d[4];
      if (MODE == FM_PAIR) {
        const float4 a = reinterpret_cast<const float4*>(L.f)[q], b = reinterpret_cast<const float4*>(L.r)[q];
        d[0] = a.x - b.x;
        d[1] = a.y - b.y;
        d[2] = a.z - b.z;
        d[3] = a.w - b.w;
      } else {
        const float4 sg = *reinterpret_cast<const float4*>(signs + L.sign0 + c0);       // the signs of a quad; 0 in the pad lanes
        d[0] = sg.x;
        d[1] = sg.y;
        d[2] = sg.z;
        d[3] = sg.w;
      }
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = c0 + j < L.c ? fm_signed(d[j], k) : 0.f;      // a pad lane: exactly 0
      g4[q] = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
static int fm_check(const char* who, const size_t* rows, const int* channels, int n_layers, int mode) {
  VCG_CHECK_ARG(mode == FM_PAIR || mode == FM_MEAN, "%s: unknown mode %d (0 pair, 1 mean)", who, mode);
  VCG_CHECK_ARG(n_layers >= 1 && n_layers <= FM_MAX_LAYERS, "%s: takes 1..%d layers, got %d", who, FM_MAX_LAYERS, n_layers);
  VCG_CHECK_ARG(rows && channels, "%s: null rows or channels table", who);
  for (int l = 0; l < n_layers; ++l) {
    VCG_CHECK_ARG(rows[l] > 0 && channels[l] > 0, "%s: layer %d is empty (rows %zu, channels %d)", who, l, rows[l], channels[l]);
    VCG_CHECK_ARG(rows[l] <= ((size_t)1 << 40) && channels[l] <= (1 << 20), "%s: layer %d is too large (rows %zu, channels %d)", who,
                  l, rows[l], channels[l]);
  }
  return 0;
}

// the geometry of all layers; chunked = the flat space is the layers' chunks (pair forward, backward), else the mean workgroups.
// `wanted`: backward only, the layers with a gradient buffer; the others take no part in the flat space.
static FmPlan fm_plan(const size_t* rows, const int* channels, int n_layers, bool chunked, float* const* wanted) {
  FmPlan p;
  p.n = n_layers;
  size_t first = 0, part = 0;
  int sign0 = 0, group0 = 0;
  for (int l = 0; l < FM_MAX_LAYERS; ++l) {
    FmLayer& L = p.l[l];
    L.f = L.r = nullptr;
    L.g = nullptr;
    if (l >= n_layers) {
      L.rows = L.n4 = L.part = L.slab = L.nslab = 0;
      L.first = first;
      L.k = 0.0;
      L.c = 0;
      L.cp4 = L.tc = L.cgroups = 1;
      L.tc_log2 = L.sign0 = 0;
      L.group0 = group0;
      continue;
    }
    L.rows = rows[l];
    L.c = channels[l];
    L.cp4 = (channels[l] + 3) / 4;
    L.n4 = L.rows * (size_t)L.cp4;
    L.k = 1.0 / ((double)n_layers * (double)L.rows * (double)L.c);
    int tc = 1, lg = 0;
    while (tc < L.cp4 && tc < FM_MAX_TC) tc *= 2, ++lg;
    L.tc = tc;
    L.tc_log2 = lg;
    L.cgroups = (L.cp4 + tc - 1) / tc;
    L.slab = (size_t)(FM_THREADS / tc) * FM_MEAN_RPL;
    L.nslab = (L.rows + L.slab - 1) / L.slab;
    L.part = part;
    L.sign0 = sign0;
    L.group0 = group0;
    L.first = first;
    part += L.nslab * (size_t)(4 * L.cp4);
    sign0 += 4 * L.cp4;
    group0 += (L.c + FM_FINAL_CW - 1) / FM_FINAL_CW;
    if (chunked)
      first += (wanted && !wanted[l]) ? 0 : (L.n4 + FM_PAIR_CHUNK - 1) / FM_PAIR_CHUNK;
    else
      first += L.nslab * (size_t)L.cgroups;
  }
  p.total = first;
  p.groups = group0;
  return p;
}

static size_t fm_blocks(size_t total) { return total < FM_MAX_BLOCKS ? total : FM_MAX_BLOCKS; }

static size_t fm_ws_bytes(const size_t* rows, const int* channels, int n_layers, int mode) {
  if (mode == FM_PAIR) return FM_MAX_BLOCKS * sizeof(double);
  const FmPlan p = fm_plan(rows, channels, n_layers, false, nullptr);
  const FmLayer& last = p.l[n_layers - 1];
  return (last.part + last.nslab * (size_t)(4 * last.cp4) + (size_t)p.groups) * sizeof(double);      // partials, then one per group
}

extern "C" size_t vcg_feature_match_chunk(int mode, int channels) {
  if ((mode != FM_PAIR && mode != FM_MEAN) || channels < 1 || channels > (1 << 20)) {
    vcg_set_error("vcg_feature_match_chunk: bad arguments (mode %d, channels %d)", mode, channels);
    return 0;
  }
  if (mode == FM_PAIR) return FM_PAIR_CHUNK;
  const size_t one = 1;
  const FmPlan p = fm_plan(&one, &channels, 1, false, nullptr);
  return p.l[0].slab;
}

extern "C" size_t vcg_feature_match_workspace(const size_t* rows, const int* channels, int n_layers, int mode) {
  if (fm_check("vcg_feature_match_workspace", rows, channels, n_layers, mode)) return 0;
  return fm_ws_bytes(rows, channels, n_layers, mode);
}

extern "C" int vcg_feature_match_fwd(const float* const* fake, const float* const* real, const size_t* rows, const int* channels,
                                     int n_layers, int mode, float* out, float* signs, void* ws, size_t ws_bytes, void* stream) {
  if (fm_check("vcg_feature_match_fwd", rows, channels, n_layers, mode)) return -1;
  VCG_CHECK_ARG(fake && real && out && ws, "vcg_feature_match_fwd: null pointer");
  VCG_CHECK_ARG(mode == FM_PAIR || (signs && ((uintptr_t)signs & 15) == 0),
                "vcg_feature_match_fwd: the mean mode needs the channel-sign buffer, 16-byte aligned");
  VCG_CHECK_ARG(((uintptr_t)ws & 15) == 0, "vcg_feature_match_fwd: workspace not 16-byte aligned");
  const size_t need = fm_ws_bytes(rows, channels, n_layers, mode);
  VCG_CHECK_ARG(ws_bytes >= need, "vcg_feature_match_fwd: workspace too small (%zu bytes, needs %zu)", ws_bytes, need);
  FmPlan p = fm_plan(rows, channels, n_layers, mode == FM_PAIR, nullptr);
  for (int l = 0; l < n_layers; ++l) {
    VCG_CHECK_ARG(fake[l] && real[l], "vcg_feature_match_fwd: layer %d has a null pointer", l);
    VCG_CHECK_ARG((((uintptr_t)fake[l] | (uintptr_t)real[l]) & 15) == 0, "vcg_feature_match_fwd: layer %d is not 16-byte aligned", l);
    p.l[l].f = fake[l];
    p.l[l].r = real[l];
  }
  hipStream_t st = (hipStream_t)stream;
  if (mode == FM_PAIR) {
    const unsigned blocks = (unsigned)fm_blocks(p.total);
    hipLaunchKernelGGL(k_fm_pair_partial, dim3(blocks), dim3(FM_THREADS), 0, st, p, (double*)ws);
    hipLaunchKernelGGL(k_fm_final, dim3(1), dim3(FM_FINAL_THREADS), 0, st, (const double*)ws, (int)blocks, out);
  } else {
    VCG_CHECK_ARG(p.total <= 0x7fffffffu, "vcg_feature_match_fwd: %zu workgroups are more than a grid holds", p.total);
    hipLaunchKernelGGL(k_fm_mean_partial, dim3((unsigned)p.total), dim3(FM_THREADS), 0, st, p, (double*)ws);
    const FmLayer& last = p.l[n_layers - 1];
    double* gpart = (double*)ws + last.part + last.nslab * (size_t)(4 * last.cp4);
    hipLaunchKernelGGL(k_fm_mean_channels, dim3((unsigned)p.groups), dim3(FM_FINAL_THREADS), 0, st, p, (const double*)ws, signs, gpart);
    hipLaunchKernelGGL(k_fm_final, dim3(1), dim3(FM_FINAL_THREADS), 0, st, (const double*)gpart, p.groups, out);
  }
  VCG_LAUNCH_CHECK("vcg_feature_match_fwd");
  return 0;
}

extern "C" int vcg_feature_match_bwd(const float* const* fake, const float* const* real, const float* signs, const float* g_out,
                                     float* const* g_fake, const size_t* rows, const int* channels, int n_layers, int mode,
                                     void* stream) {
  if (fm_check("vcg_feature_match_bwd", rows, channels, n_layers, mode)) return -1;
  VCG_CHECK_ARG(g_out && g_fake, "vcg_feature_match_bwd: null pointer");
  VCG_CHECK_ARG(mode == FM_PAIR ? (fake && real) : (signs != nullptr && ((uintptr_t)signs & 15) == 0),
                "vcg_feature_match_bwd: the pair mode needs both operand tables, the mean mode the channel signs");
  FmPlan p = fm_plan(rows, channels, n_layers, true, g_fake);
  for (int l = 0; l < n_layers; ++l) {
    if (!g_fake[l]) continue;                      // a layer that needs no gradient
    VCG_CHECK_ARG(((uintptr_t)g_fake[l] & 15) == 0, "vcg_feature_match_bwd: gradient %d is not 16-byte aligned", l);
    if (mode == FM_PAIR) {
      VCG_CHECK_ARG(fake[l] && real[l], "vcg_feature_match_bwd: layer %d has a null pointer", l);
      VCG_CHECK_ARG((((uintptr_t)fake[l] | (uintptr_t)real[l]) & 15) == 0, "vcg_feature_match_bwd: layer %d is not 16-byte aligned", l);
      p.l[l].f = fake[l];
      p.l[l].r = real[l];
    }
    p.l[l].g = g_fake[l];
  }
  if (p.total == 0) return 0;                      // no layer wants a gradient
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)fm_blocks(p.total);
  if (mode == FM_PAIR)
    hipLaunchKernelGGL(k_fm_bwd<FM_PAIR>, dim3(blocks), dim3(FM_THREADS), 0, st, p, g_out, signs);
  else
    hipLaunchKernelGGL(k_fm_bwd<FM_MEAN>, dim3(blocks), dim3(FM_THREADS), 0, st, p, g_out, signs);
  VCG_LAUNCH_CHECK("vcg_feature_match_bwd");
  return 0;
}
