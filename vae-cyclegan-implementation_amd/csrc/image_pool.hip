// Image history pool of the discriminators (Shrivastava et al. 2017, the buffer of 50 generated images every CycleGAN-style trainer
// keeps): one launch that hands each fake of a batch to the discriminator either as itself or exchanged against a stored one.  The
// host decides which (image_pool.py draws the plan); the kernel moves the words.  New: the reference has no such buffer, and a run
// without one launches nothing from this file.
//
//   vcg_pool_exchange:  for n = 0 .. N-1 in order, with p = plan[n]
//                         p == -1        keep:   out[n] = fake[n]
//                         0 <= p < cap   swap:   out[n] = pool[p], then pool[p] = fake[n]
//                         p == -(2 + s)  store:  pool[s] = fake[n], out[n] = fake[n]   (the slot's old content is not read)
//
// Two samples of one batch may name the same slot: the second receives the first one's fake.  That read-after-write is why the work
// is split over ELEMENTS and never over samples: a lane owns element index i (one 16-byte group of every image, or one word of the
// elems % 4 tail) and walks the samples of the launch in plan order for that index, so whatever is written to a slot and read again
// is written and read by the same lane in program order.  No two lanes touch the same word; nothing is synchronised.
//
// The plan travels by value in the kernel arguments (POOL_PLAN_MAX entries): no upload, no host synchronisation.  A longer batch is
// cut into launches of at most POOL_PLAN_MAX samples on the same stream, whose order keeps the sequential meaning.
//
// ema.hip's shape: four words per lane, grid-stride, at most POOL_MAX_BLOCKS workgroups of POOL_THREADS lanes, the elems % 4 last
// words of every image by workgroup 0.  Words, not floats: a NaN keeps its payload.  An image starts at a multiple of `elems` words,
// which is 16-byte aligned only where elems % 4 == 0, so a group is moved as 16 bytes of 4-byte alignment (ld4 / st4): one
// 16-byte access where the address allows it, correct where it does not.  Plain C++, vector loads and stores only.
#include "vcg_common.h"

#define POOL_THREADS 256
#define POOL_MAX_BLOCKS 2048
#define POOL_PLAN_MAX 64

struct PoolPlan {
  int32_t e[POOL_PLAN_MAX];
};

static int pool_blocks(size_t n4) {
  size_t b = (n4 + POOL_THREADS - 1) / POOL_THREADS;
  if (b > POOL_MAX_BLOCKS) b = POOL_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

__device__ __forceinline__ uint4 ld4(const uint32_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}
__device__ __forceinline__ void st4(uint32_t* p, const uint4& v) { __builtin_memcpy(p, &v, 16); }

// fake, out: the n <= POOL_PLAN_MAX images of this launch.  No __restrict__ on pool: two samples may name one slot.
__global__ __launch_bounds__(POOL_THREADS) void k_pool_exchange(const uint32_t* fake, uint32_t* pool, uint32_t* out, PoolPlan plan,
                                                                int n, size_t elems) {
  const size_t n4 = elems / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    for (int s = 0; s < n; ++s) {
      const int32_t p = plan.e[s];
      const size_t at = (size_t)s * elems + 4 * i;
      const uint4 f = ld4(fake + at);
      if (p == -1) {
        st4(out + at, f);
      } else if (p >= 0) {
        uint32_t* slot = pool + (size_t)p * elems + 4 * i;
        const uint4 old = ld4(slot);
        st4(slot, f);
        st4(out + at, old);
      } else {
        st4(pool + (size_t)(-(p + 2)) * elems + 4 * i, f);
        st4(out + at, f);
      }
    }
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < elems; i += blockDim.x) {
      for (int s = 0; s < n; ++s) {
        const int32_t p = plan.e[s];
        const size_t at = (size_t)s * elems + i;
        const uint32_t f = fake[at];
        if (p == -1) {
          out[at] = f;
        } else if (p >= 0) {
          uint32_t* slot = pool + (size_t)p * elems + i;
          const uint32_t old = *slot;
          *slot = f;
          out[at] = old;
        } else {
          pool[(size_t)(-(p + 2)) * elems + i] = f;
          out[at] = f;
        }
      }
    }
}

static bool pool_disjoint(uintptr_t a, uintptr_t abytes, uintptr_t b, uintptr_t bbytes) { return a + abytes <= b || b + bbytes <= a; }

extern "C" int vcg_pool_exchange(const float* fake, float* pool, float* out, const int32_t* plan, int N, size_t elems, int capacity,
                                 void* stream) {
  VCG_CHECK_ARG(fake && pool && out && plan, "vcg_pool_exchange: null pointer");
  VCG_CHECK_ARG((((uintptr_t)fake | (uintptr_t)pool | (uintptr_t)out) & 15) == 0, "vcg_pool_exchange: fake, pool or out not 16-byte aligned");
  VCG_CHECK_ARG(N >= 0, "vcg_pool_exchange: N=%d is negative", N);
  VCG_CHECK_ARG(capacity >= 1, "vcg_pool_exchange: capacity=%d, a pool holds at least one image", capacity);
  if (N == 0) return 0;
  VCG_CHECK_ARG(elems > 0, "vcg_pool_exchange: elems == 0 with N=%d images", N);
  VCG_CHECK_ARG(elems <= ((size_t)1 << 40) / (size_t)(N > capacity ? N : capacity), "vcg_pool_exchange: N=%d or capacity=%d images of elems=%zu are too large",
                N, capacity, elems);
  for (int n = 0; n < N; ++n) {
    const int64_t p = plan[n];
    VCG_CHECK_ARG(p == -1 || (p >= 0 && p < capacity) || (p <= -2 && -(p + 2) < capacity),
                  "vcg_pool_exchange: plan[%d]=%d is neither keep (-1), swap (slot) nor store (-(2 + slot)) with slot in [0, %d)", n, (int)p, capacity);
  }
  const uintptr_t uf = (uintptr_t)fake, uo = (uintptr_t)out, up = (uintptr_t)pool;
  const uintptr_t batch = (uintptr_t)N * elems * 4, held = (uintptr_t)capacity * elems * 4;
  VCG_CHECK_ARG(pool_disjoint(uf, batch, uo, batch) && pool_disjoint(uf, batch, up, held) && pool_disjoint(uo, batch, up, held),
                "vcg_pool_exchange: the fake, out and pool ranges overlap");
  const dim3 grid(pool_blocks(elems / 4)), block(POOL_THREADS);
  for (int n0 = 0; n0 < N; n0 += POOL_PLAN_MAX) {
    const int cnt = N - n0 < POOL_PLAN_MAX ? N - n0 : POOL_PLAN_MAX;
    PoolPlan pl;
    for (int j = 0; j < POOL_PLAN_MAX; ++j) pl.e[j] = j < cnt ? plan[n0 + j] : -1;
    hipLaunchKernelGGL(k_pool_exchange, grid, block, 0, (hipStream_t)stream, (const uint32_t*)fake + (size_t)n0 * elems, (uint32_t*)pool,
                       (uint32_t*)out + (size_t)n0 * elems, pl, cnt, elems);
    VCG_LAUNCH_CHECK("vcg_pool_exchange");
  }
  return 0;
}
