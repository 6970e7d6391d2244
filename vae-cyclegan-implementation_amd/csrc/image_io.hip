// Whole-image I/O of the translation tool (translate.py): decoded uint8 frames of any size -> the networks' pitch-4 fp32 layout,
// padded to multiples of 16 by reflection, and the way back: a window of a pitch-4 buffer -> contiguous HWC pixels.
//
// k_image_load: one workgroup per 256 consecutive pixels of one row of the PADDED output.  The source columns that segment
// maps to (reflection without repeating the edge: numpy.pad(mode="reflect"), also what the first convolution's own padding does)
// are one contiguous run of at most 256 pixels of one source row: the workgroup copies that run into LDS with aligned 32-bit
// loads (consecutive lanes, consecutive dwords), each lane then picks its 1 / 3 / 4 bytes out of LDS and stores one float4
// (r, g, b, 0) — consecutive lanes, consecutive 16-byte stores.  3 bytes in, 16 out per pixel: the store stream is 84 % of the
// traffic and sets the time.  Value: (float)v / 255.0f with a correctly rounded division (torchvision's ToTensor divides;
// v * (1 / 255) differs from it in the last bit for 126 of the 256 byte values).
//
// k_to_display_hw: metrics.hip's k_to_display over a window (top, left, H, W) of an (N, Hp, Wp, 4) buffer; the same rounding.
#include <math.h>
#include <stdint.h>

#include "vcg_common.h"

#define IO_SEG 256                         // output pixels per workgroup

struct LoadP {
  const unsigned char* src;                // (N, H, W, C) uint8
  float4* out;                             // (N, Hp, Wp, 4) fp32
  size_t src_bytes;                        // N * H * W * C
  int H, W, C, Hp, Wp, top, left;
};

__global__ __launch_bounds__(IO_SEG) void k_image_load(LoadP p) {
  __shared__ uint32_t stage[IO_SEG + 2];                           // 256 pixels x 4 bytes + the unaligned head
  const int tid = threadIdx.x, n = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * IO_SEG;
  const int x1 = min(x0 + IO_SEG, p.Wp) - 1;                       // last output column of this segment
  const int sy = reflect_idx(y - p.top, p.H);
  // source columns of the segment: reflect_idx is piecewise linear, its extremes lie at the ends or at the two folds
  const int a = reflect_idx(x0 - p.left, p.W), b = reflect_idx(x1 - p.left, p.W);
  int lo = min(a, b), hi = max(a, b);
  if (x0 <= p.left && p.left <= x1) lo = 0;
  if (x0 <= p.left + p.W - 1 && p.left + p.W - 1 <= x1) hi = p.W - 1;
  const size_t b0 = (((size_t)n * p.H + sy) * p.W + lo) * p.C;     // first byte of the run
  const size_t a0 = b0 & ~(size_t)3;
  const int head = (int)(b0 - a0), nbytes = head + (hi - lo + 1) * p.C, ndw = (nbytes + 3) >> 2;
  for (int i = tid; i < ndw; i += IO_SEG) {
    const size_t at = a0 + 4 * (size_t)i;
    uint32_t v;
    if (at + 4 <= p.src_bytes) {
      v = *(const uint32_t*)(p.src + at);
    } else {                                                       // the last dword of the whole buffer, if it is a partial one
      v = 0;
      for (int k = 0; k < 4; ++k)
        if (at + k < p.src_bytes) v |= (uint32_t)p.src[at + k] << (8 * k);
    }
    stage[i] = v;
  }
  __syncthreads();
  const int x = x0 + tid;
  if (x > x1) return;
  const unsigned char* s = (const unsigned char*)stage + head + (reflect_idx(x - p.left, p.W) - lo) * p.C;
  const unsigned char r = s[0], g = p.C == 1 ? r : s[1], bl = p.C == 1 ? r : s[2];
  p.out[((size_t)n * p.Hp + y) * p.Wp + x] = make_float4(__fdiv_rn((float)r, 255.0f), __fdiv_rn((float)g, 255.0f),
                                                         __fdiv_rn((float)bl, 255.0f), 0.f);
}

extern "C" int vcg_image_load(const unsigned char* src, float* out, int N, int H, int W, int C, int Hp, int Wp, int top, int left,
                              void* stream) {
  VCG_CHECK_ARG(src && out, "vcg_image_load: null pointer");
  VCG_CHECK_ARG(((uintptr_t)src & 3) == 0 && ((uintptr_t)out & 15) == 0, "vcg_image_load: src must be 4-byte and out 16-byte aligned");
  VCG_CHECK_ARG(N > 0 && N <= 65535 && H >= 2 && W >= 2 && H <= 65535 && W <= 65535, "vcg_image_load: bad N=%d H=%d W=%d", N, H, W);
  VCG_CHECK_ARG(C == 1 || C == 3 || C == 4, "vcg_image_load: %d source channels (1, 3 or 4)", C);
  VCG_CHECK_ARG(Hp >= H && Wp >= W && Hp <= 65535 && Wp <= 65535 && top >= 0 && left >= 0 && top + H <= Hp && left + W <= Wp,
                "vcg_image_load: the %dx%d frame at (%d, %d) leaves the %dx%d buffer", H, W, top, left, Hp, Wp);
  VCG_CHECK_ARG(top < H && Hp - H - top < H && left < W && Wp - W - left < W,
                "vcg_image_load: a border wider than the frame minus one cannot be filled by one reflection (%dx%d in %dx%d at (%d, %d))",
                H, W, Hp, Wp, top, left);
  LoadP p;
  p.src = src; p.out = (float4*)out; p.src_bytes = (size_t)N * H * W * C;
  p.H = H; p.W = W; p.C = C; p.Hp = Hp; p.Wp = Wp; p.top = top; p.left = left;
  hipLaunchKernelGGL(k_image_load, dim3((Wp + IO_SEG - 1) / IO_SEG, Hp, N), dim3(IO_SEG), 0, (hipStream_t)stream, p);
  VCG_LAUNCH_CHECK("vcg_image_load");
  return 0;
}

__device__ __forceinline__ float io_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// the window (top, left, H, W) of (N, Hp, Wp, 4) fp32 -> contiguous (N, H, W, 3): one thread per pixel, one float4 load each
__global__ __launch_bounds__(256) void k_to_display_hw(const float4* __restrict__ x, void* __restrict__ out, int H, int W, int Hp,
                                                       int Wp, int top, int left, int as_u8) {
  const int n = blockIdx.z, y = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= W) return;
  const float4 v = x[((size_t)n * Hp + top + y) * Wp + left + c];
  const size_t i = ((size_t)n * H + y) * W + c;
  const float ch[3] = {v.x, v.y, v.z};
  if (as_u8) {
    unsigned char* o = (unsigned char*)out + 3 * i;
    for (int k = 0; k < 3; ++k) {
      const double q = floor(255.0 * (double)ch[k] + 0.5);
      o[k] = (unsigned char)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
    }
  } else {
    float* o = (float*)out + 3 * i;
    for (int k = 0; k < 3; ++k) o[k] = io_clamp01(ch[k]);
  }
}

extern "C" int vcg_to_display_hw(const float* x, void* out, int N, int Hp, int Wp, int top, int left, int H, int W, int as_uint8,
                                 void* stream) {
  VCG_CHECK_ARG(x && out, "vcg_to_display_hw: null pointer");
  VCG_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0 && Hp <= 65535 && Wp <= 65535, "vcg_to_display_hw: bad N=%d H=%d W=%d", N, H, W);
  VCG_CHECK_ARG(top >= 0 && left >= 0 && top + H <= Hp && left + W <= Wp,
                "vcg_to_display_hw: the %dx%d window at (%d, %d) leaves the %dx%d buffer", H, W, top, left, Hp, Wp);
  hipLaunchKernelGGL(k_to_display_hw, dim3((W + 255) / 256, H, N), dim3(256), 0, (hipStream_t)stream, (const float4*)x, out, H, W, Hp,
                     Wp, top, left, as_uint8 ? 1 : 0);
  VCG_LAUNCH_CHECK("vcg_to_display_hw");
  return 0;
}
