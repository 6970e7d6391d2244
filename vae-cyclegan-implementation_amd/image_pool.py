"""Image history pool for a discriminator (Shrivastava et al. 2017; the 50-image buffer of CycleGAN-style trainers).

The pool keeps the last `capacity` generated images on the device.  Every new fake is shown to the discriminator either as itself
or, with probability 1/2 once the pool is full, exchanged against a random stored image, which it then replaces.  While the pool
fills, fakes are stored and shown as they are.

Two halves:
  * host, pure Python: `plan(n)` decides what happens to each of the next n samples and is the only place randomness is drawn,
    from a numpy Generator of the pool's own (never ops._RNG, the eps queue or torch's generators), so a run with a pool draws
    the same eps as one without;
  * device: `exchange(fake)` applies the plan with one `vcg_pool_exchange` launch on the current stream (csrc/image_pool.hip; the
    plan travels in the kernel arguments: no upload, no synchronisation, no copy launch of the framework's).

Plan entries (include/vcg.h): -1 keep, s >= 0 swap with slot s, -(2 + s) store into slot s.  They apply in order: two samples of
one batch may draw the same slot, and the second then receives the first one's fake."""
import ctypes
import sys

import numpy as np

KEEP = -1
POOL_SEED_STRIDE = 104729      # between the pools of one model (pool_seed)


def store(slot):
    return -(2 + int(slot))


def pool_seed(seed, index=0):
    """Seed of pool number `index` of a model whose configure_optimizers was given pool_seed=`seed`.  train.py passes
    ops.rank_seed(--seed, rank) — the derivation of the per-rank eps seeds — so every rank's pools draw their own plans; the pools
    of one model are a second stride apart."""
    return (int(seed) + POOL_SEED_STRIDE * (int(index) + 1)) & 0xFFFFFFFFFFFFFFFF


class ImagePool:
    def __init__(self, capacity, seed=0):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"ImagePool: capacity must be >= 1, got {capacity}")
        self.capacity = capacity
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.rng = np.random.Generator(np.random.Philox(self.seed))
        self.count = 0                      # slots filled so far
        self.shape = None                   # per-image shape of what is stored (the physical layout `exchange` was given)
        self.images = None                  # (capacity, elems) on the device, allocated at first use
        self.last_plan = []
        self.last_identity = True           # the last plan was keeps and stores only: out == fake for the whole batch
        self.last_drew = False              # the last plan drew from the generator (the pool was full for at least one sample)
        self._told_reset = False

    # ---- host ----------------------------------------------------------------------------------------------------------
    def plan(self, n):
        """What happens to the next n samples, in order.  Filling: store into slots count, count + 1, ... without a draw.  Full:
        swap = random() < 0.5 and, only then, slot = integers(capacity)."""
        out = []
        drew = False
        for _ in range(int(n)):
            if self.count < self.capacity:
                out.append(store(self.count))
                self.count += 1
                continue
            drew = True
            if self.rng.random() < 0.5:
                out.append(int(self.rng.integers(self.capacity)))
            else:
                out.append(KEEP)
        self.last_plan = out
        self.last_identity = all(p < 0 for p in out)
        self.last_drew = drew
        return out

    # ---- device --------------------------------------------------------------------------------------------------------
    def _physical(self, fake):
        """The contiguous buffer behind `fake` and how to view the result: the discriminators read pitch-4 NHWC images
        (ops.as_phys aliases them), anything else is taken as it lies."""
        from . import ops
        if ops.can_alias(fake):
            return ops.phys_of(fake), fake.shape[1]
        return fake.contiguous(), None

    def exchange(self, fake):
        """fake: the batch of generated images (detached) -> what the discriminator is shown.  Returns `fake` itself, with no
        launch, when every sample is kept; otherwise a new tensor of fake's shape and layout.  When `last_identity` is true the
        result equals `fake` (the launch only wrote the slots) and the caller may ignore it."""
        import torch
        from . import _native, ops
        ops._require_gpu(fake, "ImagePool.exchange")
        if fake.requires_grad:
            raise RuntimeError("ImagePool.exchange: pass fake.detach(): the pool is not differentiable")
        phys, channels = self._physical(fake)
        if phys.data_ptr() % 16:
            phys = phys.clone()
        n = phys.shape[0]
        shape = tuple(phys.shape[1:])
        if self.shape is not None and shape != self.shape:
            if not self._told_reset:
                print(f"ImagePool: the images changed from {self.shape} to {shape}: the pool starts empty again", file=sys.stderr)
                self._told_reset = True
            self.images = None
        if self.images is None:
            self.count = 0                  # nothing is stored (first use, new geometry, or plans drawn on the host alone)
        self.shape = shape
        elems = phys[0].numel() if n else int(np.prod(shape))
        plan = self.plan(n)
        if all(p == KEEP for p in plan):
            return fake
        if self.images is None:
            self.images = torch.empty((self.capacity, elems), dtype=torch.float32, device=fake.device)
        out = torch.empty_like(phys)
        arr = (ctypes.c_int32 * n)(*plan)
        _native.check(_native.lib().vcg_pool_exchange(ops._ptr(phys), ops._ptr(self.images), ops._ptr(out), arr, n, elems,
                                                      self.capacity, ops._stream()), "vcg_pool_exchange")
        return ops.logical_of(out, channels) if channels is not None else out.view(fake.shape)

    # ---- state ---------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """capacity, count, image shape, generator state and the filled slots on the CPU (synchronises)."""
        images = None
        if self.images is not None and self.count:
            images = self.images[:self.count].detach().cpu().clone()
        return {"capacity": self.capacity, "count": self.count, "shape": None if self.shape is None else list(self.shape),
                "rng": self.rng.bit_generator.state, "images": images}

    def load_state_dict(self, state, device=None):
        import torch
        if int(state["capacity"]) != self.capacity:
            raise ValueError(f"ImagePool: the saved pool holds {state['capacity']} images, this one {self.capacity}")
        count = int(state["count"])
        images = state.get("images")
        if not 0 <= count <= self.capacity or (images is not None and images.shape[0] != count):
            raise ValueError(f"ImagePool: the saved pool claims {count} images and carries "
                             f"{0 if images is None else images.shape[0]}")
        bitgen = getattr(np.random, state["rng"]["bit_generator"])()
        bitgen.state = state["rng"]
        self.rng = np.random.Generator(bitgen)
        self.shape = None if state["shape"] is None else tuple(int(s) for s in state["shape"])
        self.count = count
        self.images = None
        if count and images is not None:     # (no images: a pool that only ever planned on the host)
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device())
            elems = int(np.prod(self.shape))
            self.images = torch.empty((self.capacity, elems), dtype=torch.float32, device=device)
            self.images[:count].copy_(images.reshape(count, elems))
        self.last_plan, self.last_identity, self.last_drew = [], True, False
