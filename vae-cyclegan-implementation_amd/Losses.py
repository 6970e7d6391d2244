"""Atomic losses with the reference's class surface (Losses.py:14-121 of the reference),
each reduction a HIP kernel (wavefront shuffle -> block partial -> ordered final sum).

Only the six atomic classes (and StructuralLoss, GradientMatchingLoss and FocalFrequencyLoss, which the reference lacks) exist here: the reference's composite loss classes
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


class GANLossGenerator(nn.Module):
    """LSGAN generator terms: real -> 0, fake -> 1; returns (total, real, fake)  (reference Losses.py:67-83)."""

    def forward(self, D_real, D_fake):
        real_loss, _ = ops.mse_const(D_real, 0.0)
        fake_loss, _ = ops.mse_const(D_fake, 1.0)
        return ops.weighted_sum([real_loss, fake_loss], [1.0, 1.0]), real_loss, fake_loss


class GANLossDiscriminator(nn.Module):
    """LSGAN discriminator terms: real -> 1, fake -> 0; returns (total, real, fake)  (reference Losses.py:86-102)."""

    def forward(self, D_real, D_fake):
        real_loss, _ = ops.mse_const(D_real, 1.0)
        fake_loss, _ = ops.mse_const(D_fake, 0.0)
        return ops.weighted_sum([real_loss, fake_loss], [1.0, 1.0]), real_loss, fake_loss


class KLDivergenceLoss(nn.Module):
    """-0.5 * mean(1 + clamp(logvar) - mu^2 - exp(clamp(logvar)))  (reference Losses.py:105-121)."""

    def forward(self, mu, logvar):
        return ops.kl_loss(mu, logvar)
