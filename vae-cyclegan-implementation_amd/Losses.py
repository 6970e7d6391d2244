"""Atomic losses with the reference's class surface (Losses.py:14-121 of the reference),
each reduction a HIP kernel (wavefront shuffle -> block partial -> ordered final sum).

Only the six atomic classes (and StructuralLoss, MultiScaleStructuralLoss, GradientMatchingLoss, FocalFrequencyLoss and SlicedWassersteinLoss, which the reference lacks) exist here: the reference's composite loss classes
(Losses.py:123-379) are dead code there and are not part of the training step.
"""
import math
from typing import NamedTuple

import torch.nn as nn

from . import ops


class TranslationLoss(nn.Module):
    """mean |generated - target|  (reference Losses.py:14-24)."""

    def forward(self, generated, target):
        return ops.l1_loss(generated, target)


class CycleConsistencyLoss(nn.Module):
    """mean|F(G(x)) - x| + mean|G(F(y)) - y|  (reference Losses.py:27-39)."""

    def forward(self, x, y, FGx, GFy):
        return ops.weighted_sum([ops.l1_loss(FGx, x), ops.l1_loss(GFy, y)], [1.0, 1.0])


class IdentityLoss(nn.Module):
    """mean|F(x) - x| + mean|G(y) - y|  (reference Losses.py:42-65)."""

    def forward(self, x, y, Fx, Gy):
        return ops.weighted_sum([ops.l1_loss(Fx, x), ops.l1_loss(Gy, y)], [1.0, 1.0])


class StructuralLoss(nn.Module):
    """1 - mean SSIM(generated, target): 11 x 11 Gaussian window, the definition of the evaluator's SSIM metric without its
    clamp (new: the reference has no structural term)."""

    def forward(self, generated, target):
        return ops.ssim_loss(generated, target)


class MultiScaleStructuralLoss(nn.Module):
    """1 - mean MS-SSIM(generated, target) (Wang, Simoncelli & Bovik 2003): StructuralLoss's window over `scales` in 1..5 levels
    of a 2 x 2 mean pyramid, the contrast-structure means of the finer levels and the SSIM mean of the coarsest multiplied per
    image and channel under the customary exponents — the structure an 11 x 11 window on the full image cannot see
    (new: the reference has no multi-scale term).  The coarsest level must hold the window: min(H, W) >> (scales - 1) >= 11."""

    def __init__(self, scales=5):
        super().__init__()
        if isinstance(scales, bool) or not isinstance(scales, int) or not 1 <= scales <= ops.MSSSIM_MAX_SCALES:
            raise ValueError(f"scales must be an integer in 1..{ops.MSSSIM_MAX_SCALES}, got {scales!r}")
        self.scales = scales

    def forward(self, generated, target):
        return ops.msssim_loss(generated, target, self.scales)


class GradientMatchingLoss(nn.Module):
    """Multi-scale gradient matching (Eigen & Fergus 2015; Li & Snavely 2018): the mean absolute horizontal and vertical finite
    difference of generated - target, averaged over `scales` in 1..4 scales, scale s keeping every 2^s-th pixel of both axes
    (new: the reference has no edge term)."""

    def __init__(self, scales=4):
        super().__init__()
        if isinstance(scales, bool) or int(scales) != scales or not 1 <= int(scales) <= 4:
            raise ValueError(f"scales must be an integer in 1..4, got {scales!r}")
        self.scales = int(scales)

    def forward(self, generated, target):
        return ops.grad_match_loss(generated, target, self.scales)


class FocalFrequencyLoss(nn.Module):
    """Focal frequency loss (Jiang et al., ICCV 2021, patch_factor 1): the squared distance between the orthonormal 2-D spectra
    of generated and target, each frequency weighted by |difference|^alpha over its plane's maximum, the weight a constant for
    the gradient (new: the reference has no spectral term)."""

    def __init__(self, alpha=1.0):
        super().__init__()
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha < 0:
            raise ValueError(f"alpha must be a finite number >= 0, got {alpha!r}")
        self.alpha = float(alpha)

    def forward(self, generated, target):
        return ops.freq_loss(generated, target, self.alpha)


class ImageTerm(NamedTuple):
    """One optional reconstruction term beside the L1: weighted by `lambda_<key>` (configure_loss keyword; `--lambda_<key>` in
    train.py), reported as `loss_<key>`.  `option` is the keyword of its loss class's one constructor argument, if it has one."""
    key: str
    loss: type
    option: str = None
    default: object = None


# the order of the rows is the order in which the steps report the terms
IMAGE_TERMS = (
    ImageTerm("ssim", StructuralLoss),
    ImageTerm("grad", GradientMatchingLoss, "grad_scales", 4),
    ImageTerm("freq", FocalFrequencyLoss, "freq_alpha", 1.0),
)


class SlicedWassersteinLoss(nn.Module):
    """Sliced Wasserstein distance between the 7x7x3 patch sets of `generated` and `target` over `levels` in 1..3 levels of a
    2 x 2 box pyramid (ops.swd_loss; new: the reference has no distribution term).  It needs no pairing: a term for G(x) against
    the SET of y.

    Every call draws a fresh plan from the loss's own step counter: the per-level patch offsets from
    numpy.random.RandomState([seed, step]) on the host, the 128 unit directions on the device from vcg_randn at
    (DIRECTION_STREAM ^ seed, step * the draws of one matrix) — a seed stream of its own, so a run with the term on consumes the
    eps stream (ops.manual_seed) exactly as one with it off, and nothing crosses PCIe or synchronises.  state_dict() carries the
    seed and the counter: a resumed run continues the sequence."""
    DIRECTION_STREAM = 0x5D1CED5EED000000          # keeps the directions' Philox key apart from ops.manual_seed's small seeds
    DIRECTION_QUADS = (ops.SWD_DESC * ops.SWD_LOSS_DIRS + 3) // 4

    def __init__(self, levels=3, seed=0):
        super().__init__()
        if isinstance(levels, bool) or int(levels) != levels or not 1 <= int(levels) <= ops.SWD_LOSS_MAX_LEVELS:
            raise ValueError(f"levels must be an integer in 1..{ops.SWD_LOSS_MAX_LEVELS}, got {levels!r}")
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 32:
            raise ValueError(f"seed must be an integer in 0..2^32-1, got {seed!r}")
        self.levels = int(levels)
        self.seed = int(seed)
        self.step = 0

    def offsets(self, n_images, h, w, step=None):
        """((oy, ox) per level) of call number `step` (None: the next one) on `n_images` H x W images: uniform on [0, s_k - 7]^2."""
        import numpy as np
        rng = np.random.RandomState([self.seed, self.step if step is None else int(step)])
        return tuple((int(rng.randint(s - ops.SWD_PATCH + 1)), int(rng.randint(s - ops.SWD_PATCH + 1)))
                     for _, _, s, _ in ops.swd_loss_geometry(n_images, h, w, self.levels))

    def directions(self, device, step=None):
        """The (147, 128) unit directions of call number `step` (None: the next one), drawn and normalised on `device`."""
        step = self.step if step is None else int(step)
        gauss = ops.randn((ops.SWD_DESC, ops.SWD_LOSS_DIRS), device, self.DIRECTION_STREAM ^ self.seed, step * self.DIRECTION_QUADS)
        return ops.swd_unit_columns(gauss)

    def draw(self, generated):
        """The plan of the next call on images shaped like `generated`; advances the counter."""
        n, _, h, w = generated.shape
        plan = ops.SwdPlan(self.offsets(n, h, w), self.directions(generated.device))
        self.step += 1
        return plan

    def forward(self, generated, target):
        if generated.dim() != 4:
            raise RuntimeError(f"swd_loss: expected (N, 3, H, W) images, got shape {tuple(generated.shape)}")
        return ops.swd_loss(generated, target, self.levels, self.draw(generated))

    def get_extra_state(self):
        return {"seed": self.seed, "step": self.step, "levels": self.levels}

    def set_extra_state(self, state):
        if int(state["levels"]) != self.levels:
            raise ValueError(f"the saved sliced Wasserstein loss has {state['levels']} levels, this one {self.levels}")
        self.seed, self.step = int(state["seed"]), int(state["step"])


class GanObjective(NamedTuple):
    """The adversarial objective of the GAN models: `objective`, one of ops.GAN_OBJECTIVES — the reference's least squares, the
    hinge (Lim & Ye 2017) or the non-saturating logistic loss (Goodfellow et al. 2014) — and `label_smooth`, the one-sided label
    smoothing of the discriminator's real term (Salimans et al. 2016).  The default is the reference's objective on the
    reference's kernels (ops.mse_const); anything else goes through ops.gan_terms."""
    objective: str = "lsgan"
    label_smooth: float = 0.0


LSGAN = GanObjective()


def gan_objective(objective="lsgan", label_smooth=0.0):
    """The validated GanObjective of a loss constructor or a configure_loss call."""
    if not isinstance(objective, str) or objective not in ops.GAN_OBJECTIVES:
        raise ValueError(f"objective must be one of {', '.join(ops.GAN_OBJECTIVES)}, got {objective!r}")
    if (isinstance(label_smooth, bool) or not isinstance(label_smooth, (int, float)) or not math.isfinite(label_smooth)
            or not 0.0 <= label_smooth < 0.5):
        raise ValueError(f"label_smooth must be a finite number in [0, 0.5), got {label_smooth!r}")
    if objective == "hinge" and label_smooth != 0.0:
        raise ValueError(f"label_smooth={label_smooth!r}: the hinge objective has no target to smooth; use lsgan or logistic")
    return GanObjective(objective, float(label_smooth))


class GANLossGenerator(nn.Module):
    """Generator terms, returns (total, real, fake).  Default: LSGAN, real -> 0, fake -> 1 (reference Losses.py:67-83); another
    `objective` of ops.GAN_OBJECTIVES: that objective's generator terms from ops.gan_terms (`label_smooth` shapes the
    discriminator's real term alone; it is taken so that both classes are built from the same arguments)."""

    def __init__(self, objective="lsgan", label_smooth=0.0):
        super().__init__()
        self.config = gan_objective(objective, label_smooth)

    def forward(self, D_real, D_fake):
        if self.config == LSGAN:
            real_loss, _ = ops.mse_const(D_real, 0.0)
            fake_loss, _ = ops.mse_const(D_fake, 1.0)
        else:
            real_loss, fake_loss = ops.gan_terms(D_real, D_fake, *self.config)[0:2]
        return ops.weighted_sum([real_loss, fake_loss], [1.0, 1.0]), real_loss, fake_loss


class GANLossDiscriminator(nn.Module):
    """Discriminator terms, returns (total, real, fake).  Default: LSGAN, real -> 1, fake -> 0 (reference Losses.py:86-102);
    otherwise the discriminator terms of `objective` with the real term's target smoothed by `label_smooth`, from ops.gan_terms."""

    def __init__(self, objective="lsgan", label_smooth=0.0):
        super().__init__()
        self.config = gan_objective(objective, label_smooth)

    def forward(self, D_real, D_fake):
        if self.config == LSGAN:
            real_loss, _ = ops.mse_const(D_real, 1.0)
            fake_loss, _ = ops.mse_const(D_fake, 0.0)
        else:
            real_loss, fake_loss = ops.gan_terms(D_real, D_fake, *self.config)[2:4]
        return ops.weighted_sum([real_loss, fake_loss], [1.0, 1.0]), real_loss, fake_loss


class FeatureMatchingLoss(nn.Module):
    """Discriminator feature matching (ops.feature_matching; new: the reference has no such term): the mean over a discriminator's
    blocks of the distance between its activations on the generated and on the real batch, the real side a constant.  `mode`, one
    of ops.FM_MODES: "pair", the element-wise L1 of pix2pixHD (Wang et al. 2018) for batches whose images correspond; "mean", the
    L1 between the per-channel expected features (Salimans et al. 2016), which needs no pairing."""

    def __init__(self, mode="mean"):
        super().__init__()
        if not isinstance(mode, str) or mode not in ops.FM_MODES:
            raise ValueError(f"mode must be one of {', '.join(ops.FM_MODES)}, got {mode!r}")
        self.mode = mode

    def forward(self, fake_features, real_features):
        return ops.feature_matching(list(fake_features), list(real_features), self.mode)


class KLDivergenceLoss(nn.Module):
    """-0.5 * mean(1 + clamp(logvar) - mu^2 - exp(clamp(logvar)))  (reference Losses.py:105-121).

    `free_bits` > 0 (new: the reference has no floor; Kingma et al. 2016): the value returned is mean_c max(KL_c, free_bits), KL_c
    the mean of the same term over batch and positions of latent channel c — a channel at or below the floor is no longer
    penalised, so none is pushed to zero information.  The call then leaves `plain` (the unfloored mean, what free_bits = 0
    returns), `active` (the number of channels above the floor) and `channels` (their count) of its LAST call on the module, as
    device scalars without a gradient, for the model to report.  With the default 0 it is ops.kl_loss as before."""

    def __init__(self, free_bits=0.0):
        super().__init__()
        if isinstance(free_bits, bool) or not isinstance(free_bits, (int, float)) or not math.isfinite(free_bits) or free_bits < 0:
            raise ValueError(f"free_bits must be a finite number >= 0, got {free_bits!r}")
        self.free_bits = float(free_bits)
        self.plain = self.active = None
        self.channels = 0

    def forward(self, mu, logvar):
        if self.free_bits == 0.0:
            return ops.kl_loss(mu, logvar)
        loss, self.plain, self.active = ops.kl_free_bits(mu, logvar, self.free_bits)
        self.channels = mu.shape[1]
        return loss
