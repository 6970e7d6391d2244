// HBM-bound pieces of the training step: layout repack, the reparameterisation sampler
// (Networks.py:219-227), the loss reductions of Losses.py:14-121, the spectral-normed
// full-map conv that ends the discriminator (Networks.py:248) and torch.optim.Adam's update
// (call sites Networks.py:312,894,1928-1935).  Reductions are wavefront-shuffle (64 lanes)
// -> LDS across the block's waves -> one partial per block -> fixed-order final sum in double.
#include <stdarg.h>
#include <string.h>
#include "vcg_common.h"

// ---------------------------------------------------------------- error plumbing
static thread_local char g_err[512] = "";
void vcg_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* vcg_last_error(void) { return g_err; }
extern "C" int vcg_abi_version(void) { return VCG_ABI_VERSION; }

// ---- per-device-kernel timing (diagnostic: bench.py's roofline object) -------------------------------------------
// The training path never enables it.  Enabled, every MFMA kernel launch records two HIP events on its own launch
// stream; vcg_profile_read waits for them (the ONE place this library synchronises), sums time / FLOPs / launches per
// kernel name and returns the table as text.
#include <map>
#include <string>
#include <vector>
bool g_vcg_prof_on = false;
namespace {
struct ProfRec { const char* name; double flops; hipEvent_t e0, e1; };
std::vector<ProfRec> g_prof;
}
void vcg_prof_begin(const char* kernel, double flops, hipStream_t st) {
  ProfRec r; r.name = kernel; r.flops = flops;
  if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
  hipEventRecord(r.e0, st);
  g_prof.push_back(r);
}
void vcg_prof_end(hipStream_t st) {
  if (!g_prof.empty()) hipEventRecord(g_prof.back().e1, st);
}
extern "C" int vcg_profile_enable(int on) {
  g_vcg_prof_on = on != 0;
  return 0;
}
static std::string g_prof_text;
extern "C" long vcg_profile_read(char* buf, size_t cap) {
  struct Agg { double ms = 0, flops = 0; long n = 0; };
  if (!g_prof.empty()) {                       // fold what has been recorded since the last call into the pending text
    std::map<std::string, Agg> agg;
    for (auto& r : g_prof) {
      float ms = 0.f;
      if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
        Agg& a = agg[r.name];
        a.ms += ms; a.flops += r.flops; a.n += 1;
      }
      hipEventDestroy(r.e0); hipEventDestroy(r.e1);
    }
    g_prof.clear();
    char line[256];
    for (auto& kv : agg) {
      snprintf(line, sizeof line, "%s\t%ld\t%.6f\t%.6e\n", kv.first.c_str(), kv.second.n, kv.second.ms, kv.second.flops);
      g_prof_text += line;
    }
  }
  std::string& out = g_prof_text;
  if (!buf || cap == 0) return (long)out.size() + 1;
  const size_t n = out.size() < cap - 1 ? out.size() : cap - 1;
  memcpy(buf, out.data(), n);
  buf[n] = 0;
  out.clear();
  return (long)n;
}

static int ew_blocks(size_t work) {
  size_t b = (work + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

// ---------------------------------------------------------------- operand magnitudes for the fp16 x 2 kernels (vcg_common.h)
// 16384 slots of 64 {generation, amax bits} words (8 MB), zero at load; a slot is reused every 16384 calls — a training step of the
// largest model makes about a thousand — and a handle that old is refused (vcg_operand_amax), so no reader ever meets a reused slot.
#define VCG_AMAX_SLOTS 16384
__device__ unsigned long long g_vcg_amax_slots[VCG_AMAX_SLOTS * 64];
#include <atomic>
static std::atomic<uint64_t> g_amax_gen{0};       // the slot words carry its low 32 bits; the high bits count wrap-arounds
static unsigned long long* amax_base(int dev);
VcgAmaxOut vcg_amax_new(hipStream_t) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  unsigned long long* base = amax_base(dev);
  VcgAmaxOut o;
  uint64_t g64 = ++g_amax_gen;
  if ((uint32_t)g64 == 0) g64 = ++g_amax_gen;    // generation 0 is "never written"
  // after 2^32 generations (days of training) the 32-bit tags start over and would lose every atomicMax against what the
  // previous round left: the first call of a round on a device waits for the device and clears its slots
  static thread_local uint64_t round_seen[64] = {};
  if (base && dev >= 0 && dev < 64 && round_seen[dev] != (g64 >> 32)) {
    if (round_seen[dev] != 0 || (g64 >> 32) != 0) {
      (void)hipDeviceSynchronize();
      (void)hipMemset(base, 0, sizeof(unsigned long long) * VCG_AMAX_SLOTS * 64);
    }
    round_seen[dev] = g64 >> 32;
  }
  const uint32_t g = (uint32_t)g64;
  o.gen = g;
  o.slot = base ? base + (size_t)(g % VCG_AMAX_SLOTS) * 64 : nullptr;
  return o;
}
static unsigned long long* amax_base(int dev) {
  static thread_local unsigned long long* base[64] = {};
  if (dev < 0 || dev >= 64) return nullptr;
  if (!base[dev]) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_vcg_amax_slots)) != hipSuccess) p = nullptr;
    base[dev] = (unsigned long long*)p;
  }
  return base[dev];
}
#define VCG_HANDLE_MAGIC 0xA5ull
uint64_t vcg_amax_handle(const VcgAmaxOut& o) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return o.slot ? (VCG_HANDLE_MAGIC << 56) | ((uint64_t)(dev & 0xFF) << 40) | o.gen : 0;
}
static thread_local uint64_t t_hint_x = 0, t_hint_dy = 0, t_last_amax = 0;
uint64_t vcg_take_hint_x() { const uint64_t h = t_hint_x; t_hint_x = 0; return h; }
uint64_t vcg_take_hint_dy() { const uint64_t h = t_hint_dy; t_hint_dy = 0; return h; }
void vcg_set_last_amax(uint64_t h) { t_last_amax = h; }
extern "C" void vcg_amax_hint(uint64_t x_amax, uint64_t dy_amax) { t_hint_x = x_amax; t_hint_dy = dy_amax; }
extern "C" uint64_t vcg_amax_last(void) { const uint64_t h = t_last_amax; t_last_amax = 0; return h; }
extern "C" uint64_t vcg_amax_measure(const float* t, size_t n, void* stream) {
  if (!t || n == 0 || ((uintptr_t)t & 15)) return 0;
  const VcgAmaxOut o = vcg_amax_new((hipStream_t)stream);
  if (!o.slot || vcg_absmax_launch(t, n, o, (hipStream_t)stream)) return 0;
  return vcg_amax_handle(o);
}
// A handle is honoured while its slot is at least VCG_AMAX_MARGIN generations away from reuse.  The check runs on the host when a
// kernel is ENQUEUED; the kernel reads the slot later, by as much as the host runs ahead of the device — at most one training step
// (every step ends with a metric read-back; a step takes ~1 500 generations, side stream included), so the margin is several steps
// (round 3 had 1 024: less than one step — ADVICE r3).
#define VCG_AMAX_MARGIN 6144
static bool amax_handle_valid(uint64_t handle, int dev) {
  if ((handle >> 56) != VCG_HANDLE_MAGIC) return false;
  const uint32_t gen = (uint32_t)handle;
  const uint32_t age = (uint32_t)g_amax_gen.load() - gen;
  return (int)((handle >> 40) & 0xFF) == (dev & 0xFF) && gen != 0 && age < VCG_AMAX_SLOTS - VCG_AMAX_MARGIN;
}
extern "C" int vcg_amax_valid(uint64_t handle) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return amax_base(dev) && amax_handle_valid(handle, dev) ? 1 : 0;
}
int vcg_operand_amax(const float* t, size_t n, uint64_t handle, int shift, hipStream_t st, VcgAmax* out) {
  if ((handle >> 56) == VCG_HANDLE_MAGIC) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint32_t gen = (uint32_t)handle;
    unsigned long long* base = amax_base(dev);
    if (base && amax_handle_valid(handle, dev)) {
      VcgAmaxOut o; o.gen = gen; o.slot = base + (size_t)(gen % VCG_AMAX_SLOTS) * 64;
      *out = vcg_amax_in(o, shift);
      return 0;
    }
  }
  const VcgAmaxOut o = vcg_amax_new(st);
  if (vcg_absmax_launch(t, n, o, st)) return -2;
  *out = vcg_amax_in(o, shift);
  return 0;
}
__global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ tf, size_t n, unsigned long long* __restrict__ slot, uint32_t gen) {
  __shared__ uint32_t red[4];
  const float4* t = reinterpret_cast<const float4*>(tf);
  const size_t n4 = n / 4;
  uint32_t m = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t b = vcg_abs_bits4(t[i]);
    m = b > m ? b : m;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {                 // the tail of a tensor whose element count is not a multiple of 4
    const uint32_t b = vcg_abs_bits(tf[n4 * 4 + threadIdx.x]);
    m = b > m ? b : m;
  }
  vcg_amax_publish(m, slot, gen, red);
}
int vcg_absmax_launch(const float* t, size_t n, const VcgAmaxOut& out, hipStream_t st) {
  VCG_CHECK_ARG(t && out.slot, "absmax: null pointer (no amax slot on this device)");
  VCG_CHECK_ARG(((uintptr_t)t & 15) == 0, "absmax: the tensor must be 16-byte aligned");
  size_t blocks = (n / 4 + 1023) / 1024;                          // ~4 float4 per thread
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_absmax, dim3((unsigned)blocks), dim3(256), 0, st, t, n, out.slot, out.gen);
  VCG_LAUNCH_CHECK("absmax");
  return 0;
}

// ---------------------------------------------------------------- layout
__global__ void k_nchw_to_nhwc(const float* __restrict__ src, float* __restrict__ dst, int N, int C, int H, int W,
                               int P) {
  const size_t total = (size_t)N * H * W * P;
  const size_t HW = (size_t)H * W;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    int c = (int)(idx % P);
    size_t pixg = idx / P;
    size_t n = pixg / HW, pix = pixg - n * HW;
    dst[idx] = (c < C) ? src[(n * C + c) * HW + pix] : 0.f;
  }
}
__global__ void k_nhwc_to_nchw(const float* __restrict__ src, float* __restrict__ dst, int N, int C, int H, int W,
                               int P) {
  const size_t total = (size_t)N * C * H * W;
  const size_t HW = (size_t)H * W;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    size_t pix = idx % HW;
    size_t nc = idx / HW;
    size_t n = nc / C;
    int c = (int)(nc - n * C);
    dst[idx] = src[(n * HW + pix) * P + c];
  }
}
__global__ void k_fill(float* __restrict__ dst, float v, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = v;
}

extern "C" int vcg_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W, int P, void* stream) {
  VCG_CHECK_ARG(src && dst && N > 0 && C > 0 && H > 0 && W > 0 && P >= C, "vcg_nchw_to_nhwc: bad args");
  hipLaunchKernelGGL(k_nchw_to_nhwc, dim3(ew_blocks((size_t)N * H * W * P)), dim3(256), 0, (hipStream_t)stream, src,
                     dst, N, C, H, W, P);
  VCG_LAUNCH_CHECK("vcg_nchw_to_nhwc");
  return 0;
}
extern "C" int vcg_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, int P, void* stream) {
  VCG_CHECK_ARG(src && dst && N > 0 && C > 0 && H > 0 && W > 0 && P >= C, "vcg_nhwc_to_nchw: bad args");
  hipLaunchKernelGGL(k_nhwc_to_nchw, dim3(ew_blocks((size_t)N * H * W * C)), dim3(256), 0, (hipStream_t)stream, src,
                     dst, N, C, H, W, P);
  VCG_LAUNCH_CHECK("vcg_nhwc_to_nchw");
  return 0;
}
extern "C" int vcg_fill(float* dst, float value, size_t n, void* stream) {
  VCG_CHECK_ARG(dst || n == 0, "vcg_fill: null pointer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_fill, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, dst, value, n);
  VCG_LAUNCH_CHECK("vcg_fill");
  return 0;
}

// ---------------------------------------------------------------- Philox4x32-10 (philox4x32_10, randn4: vcg_common.h)
__global__ void k_randn(float* __restrict__ out, size_t n, uint64_t seed, uint64_t offset) {
  const size_t nq = (n + 3) / 4;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
    float4 v = randn4(seed, offset + q);
    float vv[4] = {v.x, v.y, v.z, v.w};
    for (int e = 0; e < 4; ++e)
      if (q * 4 + e < n) out[q * 4 + e] = vv[e];
  }
}
__global__ void k_rand_uniform(float* __restrict__ out, size_t n, uint64_t seed, uint64_t offset) {
  const size_t nq = (n + 3) / 4;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
    Philox4 r = philox4x32_10(offset + q, seed);
    // [0,1): torch.rand-like synthetic pixels
    float vv[4] = {(float)(r.x >> 8) * (1.0f / 16777216.0f), (float)(r.y >> 8) * (1.0f / 16777216.0f),
                   (float)(r.z >> 8) * (1.0f / 16777216.0f), (float)(r.w >> 8) * (1.0f / 16777216.0f)};
    for (int e = 0; e < 4; ++e)
      if (q * 4 + e < n) out[q * 4 + e] = vv[e];
  }
}
extern "C" int vcg_randn(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream) {
  VCG_CHECK_ARG(out || n == 0, "vcg_randn: null pointer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_randn, dim3(ew_blocks((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n, seed, offset);
  VCG_LAUNCH_CHECK("vcg_randn");
  return 0;
}
extern "C" int vcg_rand_uniform(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream) {
  VCG_CHECK_ARG(out || n == 0, "vcg_rand_uniform: null pointer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_rand_uniform, dim3(ew_blocks((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n, seed, offset);
  VCG_LAUNCH_CHECK("vcg_rand_uniform");
  return 0;
}

// ---------------------------------------------------------------- reparameterisation
__global__ void k_reparam_fwd(const float* __restrict__ mu, const float* __restrict__ lv,
                              const float* __restrict__ eps, float* __restrict__ eps_out, float* __restrict__ z,
                              float* __restrict__ lvc, size_t n, uint64_t seed, uint64_t offset) {
  const size_t nq = (n + 3) / 4;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
    float e4[4];
    if (!eps) {
      float4 v = randn4(seed, offset + q);
      e4[0] = v.x; e4[1] = v.y; e4[2] = v.z; e4[3] = v.w;
    }
    for (int e = 0; e < 4; ++e) {
      size_t i = q * 4 + e;
      if (i >= n) break;
      float ev = eps ? eps[i] : e4[e];
      float l = fminf(fmaxf(lv[i], -10.f), 10.f);
      float sd = expf(0.5f * l);
      z[i] = mu[i] + ev * sd;
      lvc[i] = l;
      if (eps_out) eps_out[i] = ev;
    }
  }
}
__global__ void k_reparam_bwd(const float* __restrict__ gz, const float* __restrict__ glvc,
                              const float* __restrict__ eps, const float* __restrict__ lv, float* __restrict__ dmu,
                              float* __restrict__ dlv, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float l = lv[i];
    float lc = fminf(fmaxf(l, -10.f), 10.f);
    float g = gz ? gz[i] : 0.f;
    float gl = g * eps[i] * 0.5f * expf(0.5f * lc) + (glvc ? glvc[i] : 0.f);
    // torch.clamp passes the gradient on the closed interval [-10, 10]
    dlv[i] = (l >= -10.f && l <= 10.f) ? gl : 0.f;
    dmu[i] = g;
  }
}
extern "C" int vcg_reparam_fwd(const float* mu, const float* lv, const float* eps, float* eps_out, float* z,
                               float* lvc, size_t n, uint64_t seed, uint64_t offset, void* stream) {
  VCG_CHECK_ARG(mu && lv && z && lvc, "vcg_reparam_fwd: null pointer");
  VCG_CHECK_ARG(eps || eps_out, "vcg_reparam_fwd: device-drawn eps must be written to eps_out for the backward");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_reparam_fwd, dim3(ew_blocks((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mu, lv, eps,
                     eps_out, z, lvc, n, seed, offset);
  VCG_LAUNCH_CHECK("vcg_reparam_fwd");
  return 0;
}
extern "C" int vcg_reparam_bwd(const float* gz, const float* glvc, const float* eps, const float* lv, float* dmu,
                               float* dlv, size_t n, void* stream) {
  VCG_CHECK_ARG(eps && lv && dmu && dlv, "vcg_reparam_bwd: null pointer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_reparam_bwd, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, gz, glvc, eps, lv, dmu,
                     dlv, n);
  VCG_LAUNCH_CHECK("vcg_reparam_bwd");
  return 0;
}

// ---------------------------------------------------------------- block reductions
__device__ static inline float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  float s = 0.f;
  const int nw = (blockDim.x + 63) >> 6;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

static const int kRedBlocks = 1024;
extern "C" size_t vcg_reduce_workspace(size_t n) {
  (void)n;
  return (size_t)kRedBlocks * 2 * sizeof(float) + 256;
}

// MODE 0: |a-b| ; MODE 1: KL term 1 + lvc - mu^2 - exp(lvc)  (a=mu, b=lv)
template <int MODE>
__global__ __launch_bounds__(256) void k_reduce_partial(const float* __restrict__ a, const float* __restrict__ b,
                                                        float* __restrict__ part, size_t n) {
  __shared__ float red[4];
  float s = 0.f;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 x = reinterpret_cast<const float4*>(a)[i];
    float4 y = reinterpret_cast<const float4*>(b)[i];
    if (MODE == 0) {
      s += fabsf(x.x - y.x) + fabsf(x.y - y.y) + fabsf(x.z - y.z) + fabsf(x.w - y.w);
    } else {
      float l;
      l = fminf(fmaxf(y.x, -10.f), 10.f); s += 1.f + l - x.x * x.x - expf(l);
      l = fminf(fmaxf(y.y, -10.f), 10.f); s += 1.f + l - x.y * x.y - expf(l);
      l = fminf(fmaxf(y.z, -10.f), 10.f); s += 1.f + l - x.z * x.z - expf(l);
      l = fminf(fmaxf(y.w, -10.f), 10.f); s += 1.f + l - x.w * x.w - expf(l);
    }
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      if (MODE == 0) s += fabsf(a[i] - b[i]);
      else { float l = fminf(fmaxf(b[i], -10.f), 10.f); s += 1.f + l - a[i] * a[i] - expf(l); }
    }
  float tot = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ void k_reduce_final(const float* __restrict__ part, int nblocks, double scale, float* __restrict__ out) {
  // one wave; fixed order
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) s += (double)part[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) out[0] = (float)(s * scale);
}

static int red_blocks(size_t n) {
  size_t b = (n / 4 + 255) / 256;
  if (b > (size_t)kRedBlocks) b = kRedBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

extern "C" int vcg_l1_fwd(const float* a, const float* b, float* out, size_t n_phys, size_t n_logical,
                          void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(a && b && out && ws && n_logical > 0, "vcg_l1_fwd: bad args");
  VCG_CHECK_ARG(ws_bytes >= vcg_reduce_workspace(n_phys), "vcg_l1_fwd: workspace too small");
  int nb = red_blocks(n_phys);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_reduce_partial<0>, dim3(nb), dim3(256), 0, st, a, b, (float*)ws, n_phys);
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(64), 0, st, (const float*)ws, nb, 1.0 / (double)n_logical, out);
  VCG_LAUNCH_CHECK("vcg_l1_fwd");
  return 0;
}
__global__ void k_l1_bwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ gout,
                         float* __restrict__ ga, float* __restrict__ gb, size_t n, float inv_n) {
  const float s = gout[0] * inv_n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float d = a[i] - b[i];
    float g = d > 0.f ? s : (d < 0.f ? -s : 0.f);
    if (ga) ga[i] = g;
    if (gb) gb[i] = -g;
  }
}
extern "C" int vcg_l1_bwd(const float* a, const float* b, const float* gout, float* ga, float* gb, size_t n_phys,
                          size_t n_logical, void* stream) {
  VCG_CHECK_ARG(a && b && gout && (ga || gb) && n_logical > 0, "vcg_l1_bwd: bad args");
  hipLaunchKernelGGL(k_l1_bwd, dim3(ew_blocks(n_phys)), dim3(256), 0, (hipStream_t)stream, a, b, gout, ga, gb,
                     n_phys, 1.0f / (float)n_logical);
  VCG_LAUNCH_CHECK("vcg_l1_bwd");
  return 0;
}

extern "C" int vcg_kl_fwd(const float* mu, const float* lv, float* out, size_t n, void* ws, size_t ws_bytes,
                          void* stream) {
  VCG_CHECK_ARG(mu && lv && out && ws && n > 0, "vcg_kl_fwd: bad args");
  VCG_CHECK_ARG(ws_bytes >= vcg_reduce_workspace(n), "vcg_kl_fwd: workspace too small");
  int nb = red_blocks(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_reduce_partial<1>, dim3(nb), dim3(256), 0, st, mu, lv, (float*)ws, n);
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(64), 0, st, (const float*)ws, nb, -0.5 / (double)n, out);
  VCG_LAUNCH_CHECK("vcg_kl_fwd");
  return 0;
}
__global__ void k_kl_bwd(const float* __restrict__ mu, const float* __restrict__ lv, const float* __restrict__ gout,
                         float* __restrict__ gmu, float* __restrict__ glv, size_t n, float inv_n) {
  const float s = gout[0] * inv_n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float l = lv[i];
    float lc = fminf(fmaxf(l, -10.f), 10.f);
    gmu[i] = mu[i] * s;
    glv[i] = (l >= -10.f && l <= 10.f) ? -0.5f * (1.f - expf(lc)) * s : 0.f;
  }
}
extern "C" int vcg_kl_bwd(const float* mu, const float* lv, const float* gout, float* gmu, float* glv, size_t n,
                          void* stream) {
  VCG_CHECK_ARG(mu && lv && gout && gmu && glv && n > 0, "vcg_kl_bwd: bad args");
  hipLaunchKernelGGL(k_kl_bwd, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, mu, lv, gout, gmu, glv, n,
                     1.0f / (float)n);
  VCG_LAUNCH_CHECK("vcg_kl_bwd");
  return 0;
}

// LSGAN: one wave handles the (B,) discriminator output
__global__ void k_mse_const_fwd(const float* __restrict__ d, float target, float* __restrict__ out, size_t n) {
  double s = 0.0, m = 0.0;
  for (size_t i = threadIdx.x; i < n; i += 64) {
    float e = d[i] - target;
    s += (double)(e * e);
    m += (double)d[i];
  }
  s = wave_sum_d(s);
  m = wave_sum_d(m);
  if (threadIdx.x == 0) {
    out[0] = (float)(s / (double)n);
    out[1] = (float)(m / (double)n);
  }
}
__global__ void k_mse_const_bwd(const float* __restrict__ d, float target, const float* __restrict__ gout,
                                float* __restrict__ gd, size_t n) {
  const float s = gout[0] * 2.0f / (float)n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    gd[i] = (d[i] - target) * s;
}
extern "C" int vcg_mse_const_fwd(const float* d, float target, float* out, size_t n, void* stream) {
  VCG_CHECK_ARG(d && out && n > 0, "vcg_mse_const_fwd: bad args");
  hipLaunchKernelGGL(k_mse_const_fwd, dim3(1), dim3(64), 0, (hipStream_t)stream, d, target, out, n);
  VCG_LAUNCH_CHECK("vcg_mse_const_fwd");
  return 0;
}
extern "C" int vcg_mse_const_bwd(const float* d, float target, const float* gout, float* gd, size_t n, void* stream) {
  VCG_CHECK_ARG(d && gout && gd && n > 0, "vcg_mse_const_bwd: bad args");
  hipLaunchKernelGGL(k_mse_const_bwd, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, d, target, gout, gd, n);
  VCG_LAUNCH_CHECK("vcg_mse_const_bwd");
  return 0;
}

struct LinComb {
  const float* s[16];
  float w[16];
  int count;
};
__global__ void k_lincomb(LinComb lc, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float acc = 0.f;
    for (int i = 0; i < lc.count; ++i) acc += lc.w[i] * lc.s[i][0];
    out[0] = acc;
  }
}
extern "C" int vcg_lincomb_fwd(const float* const* s, const float* w, int count, float* out, void* stream) {
  VCG_CHECK_ARG(s && w && out && count > 0 && count <= 16, "vcg_lincomb_fwd: bad args (count %d)", count);
  LinComb lc;
  memset(&lc, 0, sizeof(lc));
  lc.count = count;
  for (int i = 0; i < count; ++i) {
    VCG_CHECK_ARG(s[i], "vcg_lincomb_fwd: null term %d", i);
    lc.s[i] = s[i];
    lc.w[i] = w[i];
  }
  hipLaunchKernelGGL(k_lincomb, dim3(1), dim3(64), 0, (hipStream_t)stream, lc, out);
  VCG_LAUNCH_CHECK("vcg_lincomb_fwd");
  return 0;
}

// ---------------------------------------------------------------- spectral norm + full-map conv
// W is (1, C, KH, KW): a 1 x K matrix, so the power iteration collapses to two dot products.
// v stays in OIHW order (state_dict parity); wsn_k is W/sigma permuted to (kh, kw, c) = the
// NHWC order of the 16x16x512 feature map it is dotted with.
// Stage 1 (one block, the two dependent reductions): sigma, the new u, and scal = {u0 * vnorm_inv, 1 / sigma}.
__global__ __launch_bounds__(1024) void k_sn_reduce(const float* __restrict__ w, float* __restrict__ u,
                                                    const float* __restrict__ v, float* __restrict__ sigma,
                                                    float* __restrict__ scal, int K, int update_uv) {
  __shared__ float red[16];
  const float u0 = u[0];
  const float4* w4 = reinterpret_cast<const float4*>(w);
  const int K4 = K / 4;
  float wv_sum, vnorm_inv = 0.f;
  if (update_uv) {
    float s = 0.f;
    for (int k = threadIdx.x; k < K4; k += blockDim.x) {
      const float4 a = w4[k];
      const float x0 = a.x * u0, x1 = a.y * u0, x2 = a.z * u0, x3 = a.w * u0;
      s += x0 * x0 + x1 * x1 + x2 * x2 + x3 * x3;
    }
    for (int k = K4 * 4 + threadIdx.x; k < K; k += blockDim.x) { const float x = w[k] * u0; s += x * x; }
    const float nrm = sqrtf(block_sum(s, red));
    vnorm_inv = 1.0f / fmaxf(nrm, 1e-12f);
    float t = 0.f;
    for (int k = threadIdx.x; k < K4; k += blockDim.x) {
      const float4 a = w4[k];
      t += a.x * (a.x * u0 * vnorm_inv) + a.y * (a.y * u0 * vnorm_inv) + a.z * (a.z * u0 * vnorm_inv) +
           a.w * (a.w * u0 * vnorm_inv);
    }
    for (int k = K4 * 4 + threadIdx.x; k < K; k += blockDim.x) t += w[k] * (w[k] * u0 * vnorm_inv);
    wv_sum = block_sum(t, red);
  } else {
    float t = 0.f;
    for (int k = threadIdx.x; k < K; k += blockDim.x) t += w[k] * v[k];
    wv_sum = block_sum(t, red);
  }
  const float un = update_uv ? wv_sum / fmaxf(fabsf(wv_sum), 1e-12f) : u0;
  const float sg = un * wv_sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    sigma[0] = sg;
    scal[0] = u0 * vnorm_inv;
    scal[1] = sg;
    if (update_uv) u[0] = un;
  }
}
// Stage 2 (all CUs): v = w * u0 / ||w u0|| in OIHW order, wsn_k = w / sigma permuted to (kh, kw, c)
__global__ __launch_bounds__(256) void k_sn_apply(const float* __restrict__ w, float* __restrict__ v,
                                                  const float* __restrict__ scal, float* __restrict__ wsn_k, int C,
                                                  int KK, int update_uv) {
  const int K = C * KK;
  const float vs = scal[0], sg = scal[1];
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < K; k += gridDim.x * blockDim.x) {
    const float wk = w[k];
    if (update_uv) v[k] = wk * vs;
    const int c = k / KK, r = k - c * KK;  // r = kh*KW + kw
    wsn_k[(size_t)r * C + c] = wk / sg;
  }
}
extern "C" int vcg_sn_prepare(const float* w_orig_oihw, float* u, float* v, float* sigma, float* wsn_k, int C,
                              int KH, int KW, int update_uv, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(w_orig_oihw && u && v && sigma && wsn_k && C > 0 && KH > 0 && KW > 0, "vcg_sn_prepare: bad args");
  VCG_CHECK_ARG(ws && ws_bytes >= 2 * sizeof(float), "vcg_sn_prepare: needs an 8-byte workspace");
  const int K = C * KH * KW;
  hipLaunchKernelGGL(k_sn_reduce, dim3(1), dim3(1024), 0, (hipStream_t)stream, w_orig_oihw, u, (const float*)v, sigma,
                     (float*)ws, K, update_uv);
  hipLaunchKernelGGL(k_sn_apply, dim3((K + 255) / 256 < 1024 ? (K + 255) / 256 : 1024), dim3(256), 0, (hipStream_t)stream,
                     w_orig_oihw, v, (const float*)ws, wsn_k, C, KH * KW, update_uv);
  VCG_LAUNCH_CHECK("vcg_sn_prepare");
  return 0;
}

__global__ __launch_bounds__(1024) void k_fullmap_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ out,
                                                      size_t K) {
  __shared__ float red[16];
  const float* xn = x + (size_t)blockIdx.x * K;
  float s = 0.f;
  const size_t K4 = K / 4;
  for (size_t i = threadIdx.x; i < K4; i += blockDim.x) {
    float4 a = reinterpret_cast<const float4*>(xn)[i];
    float4 b = reinterpret_cast<const float4*>(w)[i];
    s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
  }
  float tot = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = tot + (bias ? bias[0] : 0.f);
}
extern "C" int vcg_fullmap_fwd(const float* x, const float* wsn_k, const float* bias, float* out, int N, size_t K,
                               void* stream) {
  VCG_CHECK_ARG(x && wsn_k && out && N > 0 && K > 0 && K % 4 == 0, "vcg_fullmap_fwd: bad args");
  hipLaunchKernelGGL(k_fullmap_fwd, dim3(N), dim3(1024), 0, (hipStream_t)stream, x, wsn_k, bias, out, K);
  VCG_LAUNCH_CHECK("vcg_fullmap_fwd");
  return 0;
}
__global__ void k_fullmap_dgrad(const float* __restrict__ g, const float* __restrict__ w, float* __restrict__ dx,
                                int N, size_t K4) {
  const size_t total = (size_t)N * K4;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    size_t n = idx / K4, k = idx - n * K4;
    float gn = g[n];
    float4 b = reinterpret_cast<const float4*>(w)[k];
    reinterpret_cast<float4*>(dx)[idx] = make_float4(gn * b.x, gn * b.y, gn * b.z, gn * b.w);
  }
}
extern "C" int vcg_fullmap_dgrad(const float* g, const float* wsn_k, float* dx, int N, size_t K, void* stream) {
  VCG_CHECK_ARG(g && wsn_k && dx && N > 0 && K % 4 == 0, "vcg_fullmap_dgrad: bad args");
  hipLaunchKernelGGL(k_fullmap_dgrad, dim3(ew_blocks((size_t)N * K / 4)), dim3(256), 0, (hipStream_t)stream, g,
                     wsn_k, dx, N, K / 4);
  VCG_LAUNCH_CHECK("vcg_fullmap_dgrad");
  return 0;
}
// stage 1: gk[k] = sum_n g[n] x[n][k]; part[block] = sum_k gk[k] * wsn[k]
__global__ __launch_bounds__(256) void k_fullmap_wgrad1(const float* __restrict__ g, const float* __restrict__ x,
                                                        const float* __restrict__ w, float* __restrict__ gk,
                                                        float* __restrict__ part, int N, size_t K) {
  __shared__ float red[4];
  float s = 0.f;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (size_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int n = 0; n < N; ++n) acc += g[n] * x[(size_t)n * K + k];
    gk[k] = acc;
    s += acc * w[k];
  }
  float tot = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// stage 2: gw_orig[oihw(k)] += (gk[k] - dot * u*v[oihw(k)]) / sigma
__global__ __launch_bounds__(256) void k_fullmap_wgrad2(const float* __restrict__ gk, const float* __restrict__ part,
                                                        int nparts, const float* __restrict__ sigma,
                                                        const float* __restrict__ u, const float* __restrict__ v,
                                                        const float* __restrict__ g, float* __restrict__ gw,
                                                        float* __restrict__ gbias, int N, int C, int KK) {
  __shared__ float dot_s;
  if (threadIdx.x < 64) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += (double)part[i];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) dot_s = (float)s;
  }
  __syncthreads();
  const float dot = dot_s, inv_sigma = 1.0f / sigma[0], u0 = u[0];
  const size_t K = (size_t)C * KK;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (size_t)gridDim.x * blockDim.x) {
    int r = (int)(k / C), c = (int)(k - (size_t)r * C);  // k = r*C + c (NHWC-K order)
    size_t o = (size_t)c * KK + r;
    gw[o] += (gk[k] - dot * u0 * v[o]) * inv_sigma;
  }
  if (gbias && blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += g[n];
    gbias[0] += s;
  }
}
static const int kFmBlocks = 256;
extern "C" int vcg_fullmap_wgrad(const float* g, const float* x, const float* wsn_k, const float* sigma,
                                 const float* u, const float* v, float* gw_orig_oihw, float* gbias, int N, int C,
                                 int KH, int KW, void* ws, size_t ws_bytes, void* stream) {
  VCG_CHECK_ARG(g && x && wsn_k && sigma && u && v && gw_orig_oihw && ws, "vcg_fullmap_wgrad: null pointer");
  VCG_CHECK_ARG(N > 0 && C > 0 && KH > 0 && KW > 0, "vcg_fullmap_wgrad: bad dims");
  const size_t K = (size_t)C * KH * KW;
  VCG_CHECK_ARG(ws_bytes >= (K + kFmBlocks) * sizeof(float), "vcg_fullmap_wgrad: workspace too small");
  float* gk = (float*)ws;
  float* part = gk + K;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_fullmap_wgrad1, dim3(kFmBlocks), dim3(256), 0, st, g, x, wsn_k, gk, part, N, K);
  hipLaunchKernelGGL(k_fullmap_wgrad2, dim3(kFmBlocks), dim3(256), 0, st, (const float*)gk, (const float*)part,
                     kFmBlocks, sigma, u, v, g, gw_orig_oihw, gbias, N, C, KH * KW);
  VCG_LAUNCH_CHECK("vcg_fullmap_wgrad");
  return 0;
}
// the same stage for patch_head.hip: gk (kh, kw, c order) and `nparts` partial dots with wsn_k in, the spectral-norm Jacobian, the
// OIHW permutation and gbias += sum of g[0 .. Ng) out — one statement of the mathematics for both heads
int vcg_sn_wgrad_finish(const float* gk, const float* part, int nparts, const float* sigma, const float* u, const float* v,
                        const float* g, int Ng, float* gw_orig_oihw, float* gbias, int C, int KK, hipStream_t st) {
  hipLaunchKernelGGL(k_fullmap_wgrad2, dim3(kFmBlocks), dim3(256), 0, st, gk, part, nparts, sigma, u, v, g, gw_orig_oihw, gbias,
                     Ng, C, KK);
  VCG_LAUNCH_CHECK("vcg_sn_wgrad_finish");
  return 0;
}

// ---------------------------------------------------------------- Adam
// torch.optim.adam._single_tensor_adam, fp32, amsgrad=False, weight_decay=0, maximize=False:
//   exp_avg.lerp_(grad, 1-beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
//   denom = exp_avg_sq.sqrt() / bias_correction2_sqrt + eps; param.addcdiv_(exp_avg, denom, value=-step_size)
// One launch over the model's flat parameter buffer: 28 B/param of HBM traffic, float4 per lane.
// exp_avg_sq' = beta2 v + (1 - beta2) (g grad_scale)^2.  gg = g * grad_scale is rounded to fp32 (torch is handed the rounded product
// too), and squaring doubles that rounding: with grad_scale = 1/3 the fp32 formula ends 3.6 U off the exact one.  Where the product
// was rounded at all (ge, its exact rounding error from one FMA, is not 0 — never for grad_scale 1 or a power of two) the update is
// evaluated in double from the unrounded product and rounded once; elsewhere it is the fp32 formula, bit for bit what it always was.
// exp_avg takes g grad_scale - m from one FMA: the product is not rounded on its way in (for grad_scale 1 or a power of two the same
// bits as gg - m).
__device__ __forceinline__ float adam_v(float v, float g, float gscale, float gg, float b2, float w2) {
  const float ge = fmaf(g, gscale, -gg);
  if (ge != 0.f) {
    const double gd = (double)g * (double)gscale;
    return (float)((double)v * (double)b2 + (double)w2 * gd * gd);
  }
  return v * b2 + w2 * gg * gg;
}
// CLIP (vcg_adam_step_clipped): clip = the four floats vcg_grad_norm left on the device (grad_clip.hip).  clip[2] != 0 (a NaN or
// Inf in the gradient): the launch writes nothing.  Otherwise gscale becomes fl32(gscale * clip[1]), one fp32 multiply, and the
// body below is the one vcg_adam_step runs: with clip[1] == 1 the same bits.
template <bool CLIP>
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g,
                                              float* __restrict__ m, float* __restrict__ v, size_t n,
                                              float step_size, float b2, float w1, float w2, float eps, float bc2_sqrt,
                                              float gscale, const float* __restrict__ clip) {
  if (CLIP) {
    if (clip[2] != 0.f) return;
    gscale = gscale * clip[1];
  }
  // w1 = 1 - beta1 and w2 = 1 - beta2 arrive rounded from DOUBLE, as torch passes them (lerp_ weight, addcmul_ value):
  // 1.f - 0.999f is 1.3e-5 away from float(1 - 0.999), and that relative error would sit in every exp_avg_sq
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
#define ADAM1(c)                                         \
    {                                                    \
      float gg = gv.c * gscale;                          \
      mv.c = mv.c + w1 * fmaf(gv.c, gscale, -mv.c);      \
      vv.c = adam_v(vv.c, gv.c, gscale, gg, b2, w2);     \
      float den = sqrtf(vv.c) / bc2_sqrt + eps;          \
      pv.c = pv.c - step_size * (mv.c / den);            \
    }
    ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      float gg = g[i] * gscale;
      float mm = m[i] + w1 * fmaf(g[i], gscale, -m[i]);
      float vv = adam_v(v[i], g[i], gscale, gg, b2, w2);
      float den = sqrtf(vv) / bc2_sqrt + eps;
      p[i] = p[i] - step_size * (mm / den);
      m[i] = mm;
      v[i] = vv;
    }
}
extern "C" int vcg_adam_step(float* p, const float* g, float* m, float* v, size_t n, float step_size, float beta1, float beta2,
                             float one_minus_beta1, float one_minus_beta2, float eps, float bc2_sqrt, float grad_scale, void* stream) {
  VCG_CHECK_ARG(p && g && m && v, "vcg_adam_step: null pointer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_adam<false>, dim3(ew_blocks(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, step_size,
                     beta2, one_minus_beta1, one_minus_beta2, eps, bc2_sqrt, grad_scale, (const float*)nullptr);
  VCG_LAUNCH_CHECK("vcg_adam_step");
  return 0;
}
extern "C" int vcg_adam_step_clipped(float* p, const float* g, float* m, float* v, size_t n, float step_size, float beta1, float beta2,
                                     float one_minus_beta1, float one_minus_beta2, float eps, float bc2_sqrt, float grad_scale,
                                     const float* clip, void* stream) {
  VCG_CHECK_ARG(p && g && m && v && clip, "vcg_adam_step_clipped: null pointer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_adam<true>, dim3(ew_blocks(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, step_size,
                     beta2, one_minus_beta1, one_minus_beta2, eps, bc2_sqrt, grad_scale, clip);
  VCG_LAUNCH_CHECK("vcg_adam_step_clipped");
  return 0;
}

// ---------------------------------------------------------------- explicit-argument forms of the amax hand-off (ABI v6, include/vcg.h)
// The operand handles travel as arguments and the handle of what the call wrote comes back through a pointer; the thread-local
// pair vcg_amax_hint / vcg_amax_last stays as the shim these forms are built on (set, call, take — all on the calling thread).
extern "C" int vcg_conv_fwd_in_h(const float* x, const float* wf, const float* bias, float* y, float* mean, float* rstd, float eps,
                                 float* saved, const int32_t* cd, void* ws, size_t ws_bytes, uint64_t x_amax, void* stream) {
  vcg_amax_hint(x_amax, 0);
  const int rc = vcg_conv_fwd_in(x, wf, bias, y, mean, rstd, eps, saved, cd, ws, ws_bytes, stream);
  vcg_amax_hint(0, 0);
  return rc;
}
extern "C" int vcg_conv_dgrad_h(const float* dy, const float* wf, float* dx, const int32_t* cd, void* ws, size_t ws_bytes,
                                uint64_t dy_amax, void* stream) {
  vcg_amax_hint(0, dy_amax);
  const int rc = vcg_conv_dgrad(dy, wf, dx, cd, ws, ws_bytes, stream);
  vcg_amax_hint(0, 0);
  return rc;
}
extern "C" int vcg_conv_wgrad_saved_h(const float* x, const float* dy, float* gw_oihw, float* gbias, const float* saved,
                                      const int32_t* cd, void* ws, size_t ws_bytes, uint64_t x_amax, uint64_t dy_amax, void* stream) {
  vcg_amax_hint(x_amax, dy_amax);
  const int rc = vcg_conv_wgrad_saved(x, dy, gw_oihw, gbias, saved, cd, ws, ws_bytes, stream);
  vcg_amax_hint(0, 0);
  return rc;
}
extern "C" int vcg_in_apply_h(const float* t, const float* mean, const float* rstd, const float* residual, float* out, int N, int H,
                              int W, int C, int post_act, int shuffle, uint64_t* out_amax, void* stream) {
  const int rc = vcg_in_apply(t, mean, rstd, residual, out, N, H, W, C, post_act, shuffle, stream);
  const uint64_t h = vcg_amax_last();
  if (out_amax) *out_amax = rc ? 0 : h;
  return rc;
}
extern "C" int vcg_in_bwd_h(const float* g, const float* t, const float* mean, const float* rstd, float* dt, int N, int H, int W,
                            int C, int epi_act, int post_act, int shuffle, void* ws, size_t ws_bytes, uint64_t* dt_amax, void* stream) {
  const int rc = vcg_in_bwd(g, t, mean, rstd, dt, N, H, W, C, epi_act, post_act, shuffle, ws, ws_bytes, stream);
  const uint64_t h = vcg_amax_last();
  if (dt_amax) *dt_amax = rc ? 0 : h;
  return rc;
}
extern "C" int vcg_act_bwd_h(const float* g, const float* t, float* dt, size_t n, int act, uint64_t* dt_amax, void* stream) {
  const int rc = vcg_act_bwd(g, t, dt, n, act, stream);
  const uint64_t h = vcg_amax_last();
  if (dt_amax) *dt_amax = rc ? 0 : h;
  return rc;
}

// ---------------------------------------------------------------- channel split / concatenation and in-place accumulation (round 4)
// The mu convolution and the first logvar convolution of the VAE bottleneck read the same map (/root/reference/Networks.py:219-222):
// they run as ONE convolution with 2 x latent output channels, whose NHWC output is split into the two tensors the reference
// returns; the backward concatenates the two gradients again, and the weight gradient of the fused kernel is added into the two
// parameters' own gradient buffers.
__global__ __launch_bounds__(256) void k_chan_split(const float4* __restrict__ src, float4* __restrict__ a, float4* __restrict__ b, size_t rows,
                                                    int ca4, int cb4) {
  const int c4 = ca4 + cb4;
  const size_t total = rows * c4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / c4;
    const int c = (int)(i - r * c4);
    const float4 v = src[i];
    if (c < ca4) a[r * ca4 + c] = v;
    else b[r * cb4 + (c - ca4)] = v;
  }
}
__global__ __launch_bounds__(256) void k_chan_cat(const float4* __restrict__ a, const float4* __restrict__ b, float4* __restrict__ dst, size_t rows,
                                                  int ca4, int cb4) {
  const int c4 = ca4 + cb4;
  const size_t total = rows * c4;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / c4;
    const int c = (int)(i - r * c4);
    dst[i] = c < ca4 ? (a ? a[r * ca4 + c] : z) : (b ? b[r * cb4 + (c - ca4)] : z);
  }
}
extern "C" int vcg_chan_split(const float* src, float* a, float* b, size_t rows, int ca, int cb, void* stream) {
  VCG_CHECK_ARG(src && a && b && rows > 0 && ca > 0 && cb > 0 && ca % 4 == 0 && cb % 4 == 0, "vcg_chan_split: bad arguments");
  hipLaunchKernelGGL(k_chan_split, dim3(ew_blocks(rows * (ca + cb) / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)src, (float4*)a,
                     (float4*)b, rows, ca / 4, cb / 4);
  VCG_LAUNCH_CHECK("vcg_chan_split");
  return 0;
}
extern "C" int vcg_chan_cat(const float* a, const float* b, float* dst, size_t rows, int ca, int cb, void* stream) {
  VCG_CHECK_ARG(dst && rows > 0 && ca > 0 && cb > 0 && ca % 4 == 0 && cb % 4 == 0, "vcg_chan_cat: bad arguments");
  hipLaunchKernelGGL(k_chan_cat, dim3(ew_blocks(rows * (ca + cb) / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)a, (const float4*)b,
                     (float4*)dst, rows, ca / 4, cb / 4);
  VCG_LAUNCH_CHECK("vcg_chan_cat");
  return 0;
}
// dst[i] += src[i]; src[i] = 0  (n a multiple of 4, both 16-byte aligned): hands a scratch gradient over to its owner and
// leaves the scratch ready for the next accumulation
__global__ __launch_bounds__(256) void k_add_into(float4* __restrict__ dst, float4* __restrict__ src, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 d = dst[i];
    const float4 s = src[i];
    d.x += s.x; d.y += s.y; d.z += s.z; d.w += s.w;
    dst[i] = d;
    src[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
extern "C" int vcg_add_into(float* dst, float* src, size_t n, void* stream) {
  VCG_CHECK_ARG(dst && src && n > 0 && n % 4 == 0 && (((uintptr_t)dst | (uintptr_t)src) & 15) == 0, "vcg_add_into: bad arguments");
  hipLaunchKernelGGL(k_add_into, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, (float4*)dst, (float4*)src, n / 4);
  VCG_LAUNCH_CHECK("vcg_add_into");
  return 0;
}
