"""Sliced Wasserstein distance (SWD) between a set of generated images and a set of real ones, on Laplacian-pyramid patches
(Karras, Aila, Laine & Lehtinen, "Progressive Growing of GANs", ICLR 2018, section 5): the evaluator's score for unpaired
runs.  It needs no pairing and no pretrained network.  Every stage runs on the device (csrc/swd.hip); this module draws the
plan and the directions on the host and keeps the descriptors between batches.  DESIGN.md, "Sliced Wasserstein distance".

Per pyramid level: `p` patches of 7x7x3 per image at host-drawn positions (the same positions for both sets), normalised per
channel over the whole set, projected on 512 host-drawn unit directions, every projection sorted over the descriptors;
swd = 1000 * mean |sorted fake - sorted real|.  Nothing here touches `ops.manual_seed` or the eps stream.
"""
import math

import numpy as np
import torch

from . import ops

NUM_DIRECTIONS = 512              # 4 repeats x 128
DIR_REPEATS = 4


def levels(S):
    """Sides of the pyramid levels of S x S images: every S / 2^k that is whole and at least 16 (256 -> 256, 128, 64, 32, 16;
    80 -> 80, 40, 20).  S < 16 is refused."""
    return ops.swd_level_sizes(S)


def patches_for(num_images, patches_per_image=128):
    """Patches per image and level: at most 16384 descriptors per set, the column a sort workgroup holds in LDS."""
    num_images = int(num_images)
    if num_images < 1 or num_images > ops.SWD_MAX_DESC:
        raise RuntimeError(f"sliced Wasserstein distance: {num_images} images (1 .. {ops.SWD_MAX_DESC})")
    if patches_per_image < 1:
        raise RuntimeError(f"sliced Wasserstein distance: patches_per_image={patches_per_image} must be at least 1")
    return min(int(patches_per_image), ops.SWD_MAX_DESC // num_images)


def plan(seed, num_images, S, patches_per_image):
    """The patch positions: one int32 array (num_images * patches_per_image, 3) of (image, top, left) rows per level, image-major
    (image i owns rows i p .. (i + 1) p - 1, so batches append), corners uniform in [0, S_k - 7]^2, from
    numpy.random.RandomState(seed)."""
    rng = np.random.RandomState(int(seed) % (1 << 32))
    n, p = int(num_images), int(patches_per_image)
    image = np.repeat(np.arange(n, dtype=np.int32), p)
    out = []
    for sk in levels(S):
        top = rng.randint(0, sk - ops.SWD_PATCH + 1, size=n * p)
        left = rng.randint(0, sk - ops.SWD_PATCH + 1, size=n * p)
        out.append(np.ascontiguousarray(np.stack([image, top.astype(np.int32), left.astype(np.int32)], axis=1)))
    return out


def directions(seed):
    """The (147, 512) fp32 projection matrix: 4 repeats of 128 Gaussian directions, every column scaled to unit 2-norm.  Its
    stream is apart from the plan's."""
    rng = np.random.RandomState([int(seed) % (1 << 32), 0x5D])
    d = rng.randn(ops.SWD_DESC, DIR_REPEATS, NUM_DIRECTIONS // DIR_REPEATS).reshape(ops.SWD_DESC, NUM_DIRECTIONS)
    d /= np.sqrt((d * d).sum(axis=0, keepdims=True))
    return np.ascontiguousarray(d.astype(np.float32))


def _finite_or_none(v):
    return float(v) if math.isfinite(v) else None


class SlicedWasserstein:
    """swd = SlicedWasserstein(S, num_images, seed); swd.add(fake_batch, real_batch) for every batch; swd.result()."""

    def __init__(self, S, num_images, seed, patches_per_image=128):
        self.sizes = levels(S)
        self.S, self.num_images = int(S), int(num_images)
        self.patches_per_image = patches_for(num_images, patches_per_image)
        self.plans = plan(seed, self.num_images, self.S, self.patches_per_image)
        self.directions = directions(seed)
        self.done = 0
        self._desc = None                            # per level: [fake, real] (num_images * p, 147) device matrices
        self._dirs = None

    def add(self, fake, real):
        """Append the descriptors of a batch: fake and real logical (nb, 3, S, S) device batches."""
        want = (3, self.S, self.S)
        if fake.dim() != 4 or real.shape != fake.shape or tuple(fake.shape[1:]) != want:
            raise RuntimeError(f"SlicedWasserstein.add: expected two (nb, 3, {self.S}, {self.S}) batches, got {tuple(fake.shape)} "
                               f"and {tuple(real.shape)}")
        nb, p, first = fake.shape[0], self.patches_per_image, self.done
        self.done += nb
        if self.done > self.num_images:              # reported by result()
            return
        rows = self.num_images * p
        if self._desc is None:
            self._desc = [[torch.empty((rows, ops.SWD_DESC), dtype=torch.float32, device=fake.device) for _ in range(2)]
                          for _ in self.sizes]
        for which, batch in enumerate((fake, real)):
            for k, level in enumerate(ops.laplacian_pyramid(batch)):
                rows_k = self.plans[k][first * p:(first + nb) * p].copy()
                rows_k[:, 0] -= first                # the image's index in this batch
                ops.swd_gather(level, rows_k, self._desc[k][which], first * p)

    def result(self):
        """{"levels": {"<side>": swd_k}, "mean": their mean, "patches_per_image", "num_images"}; a non-finite value (a constant
        channel has no deviation to divide by) is None."""
        if self.done != self.num_images:
            raise RuntimeError(f"SlicedWasserstein: {self.done} images were added, {self.num_images} were announced")
        if self._dirs is None:
            self._dirs = torch.from_numpy(self.directions).to(self._desc[0][0].device)
        dist = []
        for fake, real in self._desc:
            proj = [ops.sort_columns(ops.swd_project(ops.swd_normalize(d), self._dirs)) for d in (fake, real)]
            dist.append(ops.swd_distance(proj[0], proj[1]))
        vals = [1000.0 * float(v) for v in torch.stack(dist).cpu()]
        mean = sum(vals) / len(vals)
        return {"levels": {str(s): _finite_or_none(v) for s, v in zip(self.sizes, vals)}, "mean": _finite_or_none(mean),
                "patches_per_image": self.patches_per_image, "num_images": self.num_images}
