"""MI355X-native networks behind the reference's `Networks.py` module surface.

Class names, constructor signatures, attribute names, `forward` return order, metric keys
and state_dict keys/shapes follow the reference (file:line cited per class) so a
reference checkpoint loads and `train.py` drives these classes unchanged.  Underneath,
every block is a fused HIP launch sequence (`ops.conv_block`): implicit-GEMM / Winograd conv on the
16-bit matrix pipe with split fp32 operands (two fp16 pieces, fp32-level rounding) and a bias/activation epilogue,
two-stage InstanceNorm statistics, and a normalise(+activation)(+residual)(+PixelShuffle) store.  torch modules (`nn.Conv2d`,
`spectral_norm`) are used only as parameter containers — their forwards are never run.

Tensors crossing module boundaries keep the logical (N, C, H, W) shape and are stored
NHWC (pitch 4 for 3-channel images); NCHW-contiguous inputs are converted on entry.
"""
import contextlib
import math
from typing import NamedTuple

import torch
import torch.nn as nn
from torch.nn.utils import spectral_norm

from . import ops
from .Losses import (IMAGE_TERMS, LSGAN, CycleConsistencyLoss, FeatureMatchingLoss, GANLossDiscriminator, GANLossGenerator,
                     IdentityLoss, KLDivergenceLoss, MultiScaleStructuralLoss, SlicedWassersteinLoss, TranslationLoss, gan_objective)
from .image_pool import ImagePool, pool_seed as _pool_seed
from .optim import FusedAdam, kl_weight_at

_ACTS = {"ReLU": ops.ACT_RELU, "LeakyReLU": ops.ACT_LEAKY, "Identity": ops.ACT_NONE, "Tanh": ops.ACT_TANH, "Sigmoid": ops.ACT_SIGMOID}


def _kaiming_relu_init(module):
    """Kaiming-normal fan_out (gain sqrt 2), zero bias: reference Networks.py:168-178, 1893-1903."""
    if isinstance(module, nn.Conv2d):
        nn.init.kaiming_normal_(module.weight, mode="fan_out", nonlinearity="relu")
        if module.bias is not None:
            nn.init.zeros_(module.bias)


# --------------------------------------------------------------------------- atoms
class CaSb(nn.Module):
    """reflect conv -> [InstanceNorm] -> activation  (reference Networks.py:57-81)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=3, activation="ReLU", use_norm=True):
        super().__init__()
        if activation not in ("ReLU", "LeakyReLU", "Tanh", "Sigmoid", "Identity"):
            raise NotImplementedError("Activation not implemented")
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                              padding_mode="reflect")
        self.norm = nn.InstanceNorm2d(out_channels)
        self.activation_name = activation
        self.use_norm = use_norm
        act = _ACTS.get(activation)
        if use_norm:
            self._spec = ops.ConvSpec(in_channels, out_channels, kernel_size, stride, padding, True, 1,
                                      ops.ACT_NONE, True, act if act is not None else 0)
        else:
            self._spec = ops.ConvSpec(in_channels, out_channels, kernel_size, stride, padding, True, 1,
                                      act if act is not None else 0, False)

    def forward(self, x, defer_out=False):
        return ops.conv_block(x, self.conv.weight, self.conv.bias, self._spec, defer=defer_out)


class D(nn.Module):
    """PixelUnshuffle(2) -> reflect conv3x3 -> ReLU -> InstanceNorm  (reference Networks.py:83-96).
    The unshuffle is folded into the conv's gather addresses (K ordered (kh,kw,i,j,c))."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.PixelUnshuffle = nn.PixelUnshuffle(downscale_factor=2)
        self.conv = nn.Conv2d(in_channels * 4, out_channels, kernel_size=3, stride=1, padding=1, padding_mode="reflect")
        self.norm = nn.InstanceNorm2d(out_channels)
        self.activation = nn.ReLU(inplace=False)
        self._spec = ops.ConvSpec(in_channels * 4, out_channels, 3, 1, 1, True, 2, ops.ACT_RELU, True)

    def forward(self, x, defer_out=False):
        """`defer_out` (internal, Encoder.forward): hand the raw conv output and its statistics to the next block's gather
        instead of writing the normalised tensor (ops.conv_block, "deferred InstanceNorm")."""
        return ops.conv_block(x, self.conv.weight, self.conv.bias, self._spec, defer=defer_out)


class R(nn.Module):
    """x + IN(conv(IN(ReLU(conv(x)))))  (reference Networks.py:98-116)."""

    def __init__(self, out_channels):
        super().__init__()
        c = out_channels
        self.conv1 = nn.Conv2d(c, c, kernel_size=3, stride=1, padding=1, padding_mode="reflect")
        self.norm1 = nn.InstanceNorm2d(c)
        self.activation1 = nn.ReLU(inplace=False)
        self.conv2 = nn.Conv2d(c, c, kernel_size=3, stride=1, padding=1, padding_mode="reflect")
        self.norm2 = nn.InstanceNorm2d(c)
        self._spec1 = ops.ConvSpec(c, c, 3, 1, 1, True, 1, ops.ACT_RELU, True)
        self._spec2 = ops.ConvSpec(c, c, 3, 1, 1, True, 1, ops.ACT_NONE, True)

    def forward(self, x):
        x = ops.to_nhwc(x)
        # conv1's InstanceNorm is applied inside conv2's input gather where conv2's geometry has one (the 1024-channel Winograd
        # layers of the training sizes): h is then never written (the fused Conv + IN + act hand-off)
        n, _, hh, ww = x.shape
        defer = ops.consumer_takes_deferred(self._spec2, n, hh, ww, torch.is_grad_enabled())
        h = ops.conv_block(x, self.conv1.weight, self.conv1.bias, self._spec1, defer=defer)
        return ops.conv_block(h, self.conv2.weight, self.conv2.bias, self._spec2, residual=x)


class U(nn.Module):
    """PixelShuffle(2) -> reflect conv3x3 -> ReLU -> InstanceNorm  (reference Networks.py:118-131).

    `pre_shuffled`: the producer already stored its output through the shuffle.
    `shuffle_out`: store this block's output through the NEXT block's PixelShuffle."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.PixelShuffle = nn.PixelShuffle(upscale_factor=2)
        self.conv = nn.Conv2d(in_channels // 4, out_channels, kernel_size=3, stride=1, padding=1, padding_mode="reflect")
        self.norm = nn.InstanceNorm2d(out_channels)
        self.activation = nn.ReLU(inplace=False)
        self._spec = ops.ConvSpec(in_channels // 4, out_channels, 3, 1, 1, True, 1, ops.ACT_RELU, True)
        self._spec_shuf = None
        if out_channels % 16 == 0:
            self._spec_shuf = ops.ConvSpec(in_channels // 4, out_channels, 3, 1, 1, True, 1, ops.ACT_RELU, True,
                                           ops.ACT_NONE, True)

    def forward(self, x, pre_shuffled=False, shuffle_out=False):
        if not pre_shuffled:
            x = ops.pixel_shuffle(x)
        spec = self._spec_shuf if shuffle_out else self._spec
        if spec is None:
            raise RuntimeError("shuffle_out needs out_channels % 16 == 0")
        return ops.conv_block(x, self.conv.weight, self.conv.bias, spec)


class S(nn.Module):
    """bare reflect conv3x3  (reference Networks.py:133-140)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, padding_mode="reflect")
        self._spec = ops.ConvSpec(in_channels, out_channels, 3, 1, 1, True, 1)

    def forward(self, x):
        return ops.conv_block(x, self.conv.weight, self.conv.bias, self._spec)


class L(S):
    """bare reflect conv3x3  (reference Networks.py:142-149)."""


# --------------------------------------------------------------------------- molecules
class Encoder(nn.Module):
    """3 -> 1024 channels at 1/16 resolution  (reference Networks.py:154-181)."""

    def __init__(self):
        super().__init__()
        self.model = nn.Sequential(CaSb(3, 64, kernel_size=7, stride=1), D(64, 128), D(128, 256), D(256, 512),
                                   D(512, 1024), R(1024))
        self.apply(self._init_weights)

    def _init_weights(self, module):
        _kaiming_relu_init(module)

    def forward(self, x):
        out = ops.to_nhwc(x)
        layers = list(self.model)
        for i, layer in enumerate(layers):
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            if isinstance(layer, (CaSb, D)) and isinstance(nxt, D):
                # the next D block normalises this block's raw output in its own gather where its geometry can (the Winograd
                # input transform: D2..D4 at the training sizes) — the normalised tensor is then never written
                n, _, hh, ww = out.shape
                ho, wo = layer._spec.out_hw(hh, ww)
                defer = layer._spec.norm and ops.consumer_takes_deferred(nxt._spec, n, ho, wo, torch.is_grad_enabled())
                out = layer(out, defer_out=defer)
            else:
                out = layer(out)
        return out


class Decoder(nn.Module):
    """mirror of Encoder  (reference Networks.py:183-211).  U->U hand-offs are stored pre-shuffled."""

    def __init__(self):
        super().__init__()
        self.model = nn.Sequential(R(1024), U(1024, 512), U(512, 256), U(256, 128), U(128, 64),
                                   CaSb(64, 3, kernel_size=7, stride=1, activation="Identity", use_norm=False))
        self.apply(self._init_weights)

    def _init_weights(self, module):
        _kaiming_relu_init(module)

    def forward(self, x):
        layers = list(self.model)
        out = ops.to_nhwc(x)
        pre = False
        for i, layer in enumerate(layers):
            if isinstance(layer, U):
                nxt = layers[i + 1] if i + 1 < len(layers) else None
                fuse = isinstance(nxt, U) and layer._spec_shuf is not None
                out = layer(out, pre_shuffled=pre, shuffle_out=fuse)
                pre = fuse
            else:
                out = layer(out)
                pre = False
        return out


class VariationalEncoderBlock(nn.Module):
    """mu / logvar convs, clamp, z = mu + eps * exp(0.5 logvar)  (reference Networks.py:214-227)."""

    def __init__(self, in_channels, latent_dim=64):
        super().__init__()
        self.muConv = L(in_channels, latent_dim)
        self.logvarConv = nn.Sequential(S(in_channels, latent_dim), S(latent_dim, latent_dim))
        self.latent_dim = latent_dim
        # mu and the first logvar convolution read the same map: one convolution with 2 x latent outputs (ops.FusedConvPair;
        # the parameters, state_dict names and optimizer entries stay the reference's)
        self._pair = None
        if latent_dim % 4 == 0:
            object.__setattr__(self, "_pair", ops.FusedConvPair(self.muConv.conv, self.logvarConv[0].conv,
                                                                ops.ConvSpec(in_channels, 2 * latent_dim, 3, 1, 1, True, 1)))

    def latent(self, x):
        """(mu, raw logvar) of `forward`'s convolutions, without the reparameterisation: no eps draw is consumed."""
        x = ops.to_nhwc(x)
        if ops.FUSE_MU_LOGVAR and self._pair is not None and x.is_cuda:
            mu, lv0 = ops.conv_pair(x, self._pair)
            return mu, self.logvarConv[1](lv0)
        return self.muConv(x), self.logvarConv(x)

    def forward(self, x):
        x = ops.to_nhwc(x)
        if ops.FUSE_MU_LOGVAR and self._pair is not None and x.is_cuda:
            mu, lv0 = ops.conv_pair(x, self._pair)
            logvar = self.logvarConv[1](lv0)
            eps = ops.next_eps(mu.shape, mu.device)
            z, logvar = ops.reparameterize(mu, logvar, eps)
            return z, mu, logvar
        mu = self.muConv(x)
        logvar = self.logvarConv(x)
        eps = ops.next_eps(mu.shape, mu.device)
        z, logvar = ops.reparameterize(mu, logvar, eps)
        return z, mu, logvar


class VariationalDecoderBlock(nn.Module):
    """latent -> 1024 channels  (reference Networks.py:230-237)."""

    def __init__(self, latent_dim=64, out_channels=1024):
        super().__init__()
        self.conv = S(latent_dim, out_channels)

    def forward(self, z):
        return self.conv(z)


class Discriminator(nn.Module):
    """4x (conv4x4 s2 [+IN] + LeakyReLU 0.2) + spectral-normed 16x16 conv, flattened (reference Networks.py:240-269): one
    logit per image at 256x256, and a patch discriminator above it — (H/16 - 15)(W/16 - 15) logits per image, n-major
    (ops.head_output_shape).  The losses and the d_*_mean metrics are means over all logits, as the reference's are."""

    def __init__(self):
        super().__init__()
        self.model = nn.Sequential(
            CaSb(3, 64, kernel_size=4, stride=2, padding=1, activation="LeakyReLU", use_norm=False),
            CaSb(64, 128, kernel_size=4, stride=2, padding=1, activation="LeakyReLU"),
            CaSb(128, 256, kernel_size=4, stride=2, padding=1, activation="LeakyReLU"),
            CaSb(256, 512, kernel_size=4, stride=2, padding=1, activation="LeakyReLU"),
            spectral_norm(nn.Conv2d(512, 1, kernel_size=16, stride=1, padding=0)),
        )
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.Conv2d):
            nn.init.kaiming_normal_(module.weight, mode="fan_out", nonlinearity="leaky_relu", a=0.2)
            if module.bias is not None:
                nn.init.zeros_(module.bias)

    def forward(self, x):
        x = ops.to_nhwc(x)
        layers = list(self.model)
        for blk in layers[:-1]:
            x = blk(x)
        head = layers[-1]
        return ops.fullmap_sn_conv(x, head.weight_orig, head.bias, head.weight_u, head.weight_v, self.training)

    def features(self, x):
        """-> ([a1, a2, a3, a4], logits) from one pass: the outputs of the four CaSb blocks (after InstanceNorm and LeakyReLU) that
        `forward` hands from block to block, and its logits — the same launches, the same bits.  What the feature-matching term
        compares (_GanMixin._add_fm)."""
        x = ops.to_nhwc(x)
        layers = list(self.model)
        acts = []
        for blk in layers[:-1]:
            x = blk(x)
            acts.append(x)
        head = layers[-1]
        return acts, ops.fullmap_sn_conv(x, head.weight_orig, head.bias, head.weight_u, head.weight_v, self.training)


# --------------------------------------------------------------------------- composites
def _metrics_to_host(named, reducer=None):
    """One device->host copy for all the step's scalars (the reference does one .item() each).
    Under data parallelism the scalars are first averaged over ranks (= the global-batch means)."""
    keys = list(named.keys())
    vec = torch.stack([named[k].detach().reshape(()) for k in keys])
    if reducer is not None:
        vec = reducer.average_metrics(vec)
    return dict(zip(keys, vec.tolist()))


def _max_grad_norm(clip_grad_norm):
    """configure_optimizers(clip_grad_norm=c) -> FusedAdam's max_grad_norm: 0.0 is off (None: the optimizer allocates and launches
    nothing new); FusedAdam refuses a negative or non-finite bound."""
    c = float(clip_grad_norm)
    return None if c == 0.0 else c


def _ema_decay(ema_decay):
    """configure_optimizers(ema_decay=d) -> FusedAdam's ema_decay: 0.0 is off (None: the optimizer allocates and launches nothing
    new); anything else must be finite and lie in [0, 1)."""
    d = float(ema_decay)
    if not math.isfinite(d) or not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay must be finite and lie in [0, 1) (0 switches the averaged weights off), got {ema_decay!r}")
    return None if d == 0.0 else d


def _pool_size(pool_size):
    """configure_optimizers(pool_size=n) -> the capacity of each discriminator's image history pool: an integer >= 0, 0 is off (no
    pool object exists and the step allocates, launches and draws nothing new)."""
    if isinstance(pool_size, bool) or int(pool_size) != pool_size or int(pool_size) < 0:
        raise ValueError(f"pool_size must be an integer >= 0 (0 switches the image history pool off), got {pool_size!r}")
    return int(pool_size)


def _refuse_pool(model, pool_size):
    """The models without a discriminator take the keyword so that one call fits every architecture: 0 is ignored."""
    if _pool_size(pool_size) != 0:
        raise ValueError(f"pool_size={pool_size}: {type(model).__name__} has no discriminator to keep an image history pool for "
                         "(cyclevaegan, cycleaegan, aegan and vaegan have)")


class _PoolMixin:
    """Image history pools (image_pool.ImagePool) of a model whose configure_optimizers was given pool_size > 0: one per
    discriminator, under the discriminator's attribute name.  `image_pools` is None otherwise.

    The step with pools: forward and the shared discriminator pass as without (the G phase is untouched), then each pool exchanges
    its discriminator's fakes on the main stream.  A discriminator whose plan was an identity (keeps and stores only: the whole
    filling phase) takes its weight gradients from the shared pass, exactly the step without a pool.  Otherwise its fake term
    comes from one more ordinary call D(pooled) on the whole batch, after the fake and the real call of the shared pass (spectral
    norm's power iteration advances per call), and the shared pass still provides the real term.

    Under data parallelism the ranks draw different plans, and a discriminator's backward nodes run in another order with the
    extra call than without it, so the order in which gradient buckets complete would differ between ranks: there every rank takes
    the extra call whenever its pool drew at all (`last_drew`: the pool is full — the same steps on every rank, their shards being
    equal), kept samples included."""
    image_pools = None
    debug_mode = False

    def _make_pools(self, names, pool_size, pool_seed):
        size = _pool_size(pool_size)
        self.image_pools = {n: ImagePool(size, _pool_seed(pool_seed, i)) for i, n in enumerate(names)} if size else None

    @property
    def pool_enabled(self):
        return bool(self.image_pools)

    def _shown_to(self, name, fake):
        """(pooled batch, whether discriminator `name` needs the extra call on it) for this step's `fake`."""
        pool = self.image_pools[name]
        shown = pool.exchange(fake)
        extra = pool.last_drew if self.grad_reducer is not None else not pool.last_identity
        return shown, extra

    def _debug_store(self):
        return self.__dict__.setdefault("debug_info", {})

    def save_pool_state(self):
        """{discriminator name: ImagePool.state_dict()} — what a checkpoint stores under `vcg_image_pool`."""
        if not self.image_pools:
            raise RuntimeError("save_pool_state(): this model keeps no image history pool (configure_optimizers(pool_size=...))")
        return {n: p.state_dict() for n, p in self.image_pools.items()}

    def load_pool_state(self, state, device=None):
        if not self.image_pools:
            raise RuntimeError("load_pool_state(): this model keeps no image history pool (configure_optimizers(pool_size=...))")
        if set(state) != set(self.image_pools):
            raise KeyError(f"saved image pools {sorted(state)} do not match this model's {sorted(self.image_pools)}")
        for n, p in self.image_pools.items():
            p.load_state_dict(state[n], device=device)


def _clip_scalars(**optimizers):
    """{suffix: optimizer} -> the device scalars a clipping optimizer's last step left in `clip_state`, under the metric names
    grad_norm<suffix> / grad_skipped<suffix> ("" for the one-optimizer models, "_G" / "_D" otherwise); {} when clipping is off.
    They join the vector _metrics_to_host copies: still one device->host copy per step.  Under data parallelism every rank holds
    the same values after the all-reduce, so the rank average returns them unchanged."""
    out = {}
    for sfx, opt in optimizers.items():
        state = getattr(opt, "clip_state", None)
        if state is not None:
            out["grad_norm" + sfx] = state[0]
            out["grad_skipped" + sfx] = state[2]
    return out


def _image_terms(kwargs):
    """The optional image terms a configure_loss call switches on: ((reported name, weight, loss module), ...) for the rows of
    Losses.IMAGE_TERMS whose lambda_<key> is > 0, in the table's order, then the multi-scale structural term (lambda_msssim,
    msssim_scales; reported as loss_msssim).  With a weight at its default 0 no loss object exists (the term's option is then not
    looked at) and the step computes, launches and reports exactly what it did before the term was added."""
    active = []
    for row in IMAGE_TERMS:
        lam = float(kwargs.get(f"lambda_{row.key}", 0.0))
        if lam < 0.0:
            raise ValueError(f"lambda_{row.key} must be >= 0, got {lam}")
        if lam > 0.0:
            option = () if row.option is None else (kwargs.get(row.option, row.default),)
            active.append((f"loss_{row.key}", lam, row.loss(*option)))
    lam = float(kwargs.get("lambda_msssim", 0.0))
    if not math.isfinite(lam) or lam < 0.0:
        raise ValueError(f"lambda_msssim must be finite and >= 0, got {lam}")
    if lam > 0.0:
        active.append(("loss_msssim", lam, MultiScaleStructuralLoss(kwargs.get("msssim_scales", 5))))
    return tuple(active)


def _eval_image_terms(terms, pairs):
    """The active terms (_image_terms) on the (generated, target) pairs, in the order they are reported: {name: device scalar} and
    their weights.  One pair: the loss module's own output; two (the cycle models): their sum."""
    named, weights = {}, []
    for name, lam, fn in terms:
        values = [fn(generated, target) for generated, target in pairs]
        named[name] = values[0] if len(values) == 1 else ops.weighted_sum(values, [1.0] * len(values))
        weights.append(lam)
    return named, weights


SWD_MODELS = "cycleae, cyclevae, cycleaegan and cyclevaegan"      # the models with two translation directions and two image sets


def _swd_weight(kwargs):
    lam = float(kwargs.get("lambda_swd", 0.0))
    if not math.isfinite(lam) or lam < 0.0:
        raise ValueError(f"lambda_swd must be finite and >= 0, got {lam}")
    return lam


def _refuse_swd(model, kwargs):
    """configure_loss of the single-direction models takes the keyword so that one call fits every architecture: 0 is ignored."""
    lam = _swd_weight(kwargs)
    if lam != 0.0:
        raise ValueError(f"lambda_swd={lam}: {type(model).__name__} translates in one direction; the sliced Wasserstein term is "
                         f"built into {SWD_MODELS}")


class _SwdMixin:
    """The sliced Wasserstein term of a cycle model whose configure_loss was given lambda_swd > 0: lambda_swd (swd(G(x), y) +
    swd(F(y), x)), a distance between the patch distributions of the translated batch and of the other domain's batch
    (Losses.SlicedWassersteinLoss).  It is the one term of the unpaired objectives that looks at G(x) against domain Y without a
    discriminator.  With the weight at its default 0 `swd_term` is None: no loss object exists, and the step computes, launches,
    draws and reports exactly what it did before the term was added."""
    swd_term = None                               # (weight, SlicedWassersteinLoss)

    def _configure_swd(self, kwargs):
        lam = _swd_weight(kwargs)
        self.swd_term = None if lam == 0.0 else (lam, SlicedWassersteinLoss(levels=kwargs.get("swd_levels", 3),
                                                                              seed=kwargs.get("swd_seed", 0)))

    @property
    def swd_enabled(self):
        return self.swd_term is not None

    def _add_swd(self, t, terms, weights, Gx, Fy, x, y):
        """Appends the term to the generator objective's (terms, weights) and to the step's scalars `t`; on the main stream, after
        the direction join."""
        if self.swd_term is not None:
            lam, fn = self.swd_term
            t["loss_swd"] = ops.weighted_sum([fn(Gx, y), fn(Fy, x)], [1.0, 1.0])
            terms.append(t["loss_swd"])
            weights.append(lam)

    def _swd_spec(self):
        return _same("loss_swd") if self.swd_term is not None else ()

    def save_swd_state(self):
        """The loss's seed and step counter — what a checkpoint stores under `vcg_swd_loss`."""
        if self.swd_term is None:
            raise RuntimeError("save_swd_state(): this model has no sliced Wasserstein term (configure_loss(lambda_swd=...))")
        return self.swd_term[1].state_dict()

    def load_swd_state(self, state):
        if self.swd_term is None:
            raise RuntimeError("load_swd_state(): this model has no sliced Wasserstein term (configure_loss(lambda_swd=...))")
        self.swd_term[1].load_state_dict(state)


KL_MODELS = "vae, vaegan, cyclevae, cyclevaegan and doublevae"      # the models with a latent distribution and a KL term


class KlControl(NamedTuple):
    """configure_loss's keywords that shape the KL term of a variational model beyond its weight lambda_kl.  kl_free_bits: the
    free-bits floor per latent channel (Losses.KLDivergenceLoss); kl_anneal_steps, kl_cycles, kl_ramp: the schedule of the weight
    over the generator optimizer's steps (optim.kl_weight_at).  The defaults switch both off: the step then computes, launches
    and reports exactly what it did before the options existed."""
    free_bits: float = 0.0
    anneal_steps: int = 0
    cycles: int = 1
    ramp: float = 1.0


_KL_OFF = KlControl()


def _kl_control(kwargs):
    """The validated KlControl of a configure_loss call."""
    def number(name, default):
        v = kwargs.get(name, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        return v

    def integer(name, default, least):
        v = number(name, default)
        if int(v) != v or int(v) < least:
            raise ValueError(f"{name} must be an integer >= {least}, got {v!r}")
        return int(v)

    free_bits = float(number("kl_free_bits", 0.0))
    if free_bits < 0.0:
        raise ValueError(f"kl_free_bits must be >= 0 (0: no floor), got {free_bits}")
    steps = integer("kl_anneal_steps", 0, 0)
    cycles = integer("kl_cycles", 1, 1)
    ramp = float(number("kl_ramp", 1.0))
    if not 0.0 < ramp <= 1.0:
        raise ValueError(f"kl_ramp must lie in (0, 1], got {ramp}")
    return KlControl(free_bits, steps, cycles, ramp)


def _refuse_kl_control(model, kwargs):
    """configure_loss of the models without a latent distribution takes the keywords so that one call fits every architecture:
    the defaults are ignored."""
    control = _kl_control(kwargs)
    if control != _KL_OFF:
        given = ", ".join(f"kl_{k}={v}" for k, v, d in zip(control._fields, control, _KL_OFF) if v != d)
        raise ValueError(f"{given}: {type(model).__name__} has no KL term to control ({KL_MODELS} have)")


def _configure_kl(model, kwargs):
    """-> the KL loss module of a variational model's configure_loss; leaves `kl_control` and `lambda_kl` on the model."""
    model.kl_control = _kl_control(kwargs)
    model.lambda_kl = kwargs.get("lambda_kl", 1e-5)
    return KLDivergenceLoss(model.kl_control.free_bits)


def _kl_weight(model, training):
    """The weight of the KL term in this step's G_loss.  A training step of a model that anneals reads the schedule at the number
    of steps its generator optimizer has completed (checkpoints restore that counter, so a resumed run continues the schedule) and
    leaves the value in `kl_weight_used` for the report; validation always weighs with the full lambda_kl, so its losses mean
    the same in every epoch.  A Python float either way, as lambda_kl is."""
    control = getattr(model, "kl_control", _KL_OFF)
    if not training or control.anneal_steps == 0:
        return model.lambda_kl
    opt = getattr(model, "optimizer_G", None)
    if opt is None:
        opt = model.optimizer
    model.kl_weight_used = kl_weight_at(model.lambda_kl, opt.step_count, control.anneal_steps, control.cycles, control.ramp)
    return model.kl_weight_used


def _kl_terms(fn, pairs):
    """The KL loss module `fn` on the (mu, logvar) pairs of a step -> (the step's KL scalars, the term that enters G_loss, the
    plain KL of every pair).  Without a floor: {"loss_kl": the sum over the pairs}, which is also the objective.  With one: loss_kl
    stays the plain sum — the number that is comparable across runs —, loss_kl_fb is the sum of the floored terms and the
    objective, kl_active the fraction of channels above the floor, averaged over the pairs."""
    def total(values):
        return values[0] if len(values) == 1 else ops.weighted_sum(values, [1.0] * len(values))

    if fn.free_bits == 0.0:
        values = [fn(mu, logvar) for mu, logvar in pairs]
        t = {"loss_kl": total(values)}
        return t, t["loss_kl"], values
    floored, plains, actives, fractions = [], [], [], []
    for mu, logvar in pairs:
        floored.append(fn(mu, logvar))
        plains.append(fn.plain)
        actives.append(fn.active)
        fractions.append(1.0 / (fn.channels * len(pairs)))
    t = {"loss_kl": total(plains), "loss_kl_fb": total(floored), "kl_active": ops.weighted_sum(actives, fractions)}
    return t, t["loss_kl_fb"], plains


def _kl_keys(model, spec, training):
    """`spec` (_report) with the keys the KL options add, directly after loss_kl: loss_kl_fb and kl_active with a floor, then
    kl_weight (a host value: `_kl_host`) in the training steps of a model that anneals.  Unchanged with the options off."""
    control = getattr(model, "kl_control", _KL_OFF)
    extra = (_same("loss_kl_fb", "kl_active") if control.free_bits > 0.0 else ()) \
        + ((("kl_weight", None),) if training and control.anneal_steps else ())
    if not extra:
        return spec
    at = [name for name, _ in spec].index("loss_kl") + 1
    return spec[:at] + extra + spec[at:]


def _kl_host(model, training):
    """_report's keyword for the kl_weight entry of `_kl_keys`: the weight the step used; it never was on the device."""
    control = getattr(model, "kl_control", _KL_OFF)
    return {"kl_weight": float(model.kl_weight_used)} if training and control.anneal_steps else {}


GAN_MODELS = "aegan, vaegan, cycleaegan and cyclevaegan"      # the models with a discriminator and an adversarial objective


def _gan_objective(kwargs):
    """The validated Losses.GanObjective of a configure_loss call (gan_objective, gan_label_smooth)."""
    return gan_objective(kwargs.get("gan_objective", "lsgan"), kwargs.get("gan_label_smooth", 0.0))


def _refuse_gan_objective(model, kwargs):
    """configure_loss of the models without a discriminator takes the keywords so that one call fits every architecture: the
    defaults are ignored."""
    config = _gan_objective(kwargs)
    if config != LSGAN:
        given = ", ".join(f"gan_{k}={v!r}" for k, v, d in zip(config._fields, config, LSGAN) if v != d)
        raise ValueError(f"{given}: {type(model).__name__} has no discriminator and no adversarial objective ({GAN_MODELS} have)")


def _configure_gan(model, kwargs):
    """-> the (generator, discriminator) loss modules of a GAN model's configure_loss; leaves `gan_objective` on the model."""
    model.gan_objective = _gan_objective(kwargs)
    return GANLossGenerator(*model.gan_objective), GANLossDiscriminator(*model.gan_objective)


def _fm_config(kwargs):
    """The validated (lambda_fm, fm_mode) of a configure_loss call."""
    lam, mode = kwargs.get("lambda_fm", 0.0), kwargs.get("fm_mode", "mean")
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not math.isfinite(lam) or lam < 0.0:
        raise ValueError(f"lambda_fm must be finite and >= 0, got {lam!r}")
    if not isinstance(mode, str) or mode not in ops.FM_MODES:
        raise ValueError(f"fm_mode must be one of {', '.join(ops.FM_MODES)}, got {mode!r}")
    return float(lam), mode


def _refuse_fm(model, kwargs):
    """configure_loss of the models without a discriminator takes the keywords so that one call fits every architecture: a weight
    of 0 is ignored."""
    lam, _ = _fm_config(kwargs)
    if lam != 0.0:
        raise ValueError(f"lambda_fm={lam}: {type(model).__name__} has no discriminator whose features could be matched "
                         f"({GAN_MODELS} have)")


class _GanTerms:
    """The adversarial terms of one discriminator's logits on real and on generated images (either may be None) under a model's
    objective, each a (term, logit mean) pair.  LSGAN without smoothing: every term is its own ops.mse_const call, issued where
    the step asks for it — call for call and launch for launch the step as it was before the objective could be chosen.  Any
    other objective: ONE ops.gan_terms call here serves all four terms and both means."""

    def __init__(self, config, real, fake):
        self.real, self.fake = real, fake
        self.fused = None if config == LSGAN else ops.gan_terms(real, fake, *config)

    def g_real(self):
        return ops.mse_const(self.real, 0.0) if self.fused is None else (self.fused[0], self.fused[4])

    def g_fake(self):
        return ops.mse_const(self.fake, 1.0) if self.fused is None else (self.fused[1], self.fused[5])

    def d_real(self):
        return ops.mse_const(self.real, 1.0) if self.fused is None else (self.fused[2], self.fused[4])

    def d_fake(self):
        return ops.mse_const(self.fake, 0.0) if self.fused is None else (self.fused[3], self.fused[5])


def _backward_and_step(loss, optimizer, reducer):
    """zero_grad -> backward -> [data-parallel gradient exchange, its buckets launched from inside the backward] -> step."""
    optimizer.zero_grad()
    if reducer is not None:
        reducer.begin(optimizer)
    ops.backward_overlapped(loss)
    if reducer is not None:
        reducer.start(optimizer)
        reducer.finish(optimizer)
    optimizer.step()


def _refuse_training_in_ema_scope(model):
    """First line of every training_step (a caller's stand-in for `self` need not know the attribute)."""
    if getattr(model, "_ema_in_scope", False):
        raise RuntimeError("training_step inside ema_scope(): the parameters hold the averaged weights; leave the scope first")


class _EmaMixin:
    """Averaged generator weights of a model whose configure_optimizers was given ema_decay > 0.  The average follows the
    optimizer that trains generators — `optimizer_G` of the GAN models, `optimizer` of the others — and lives in that optimizer
    (FusedAdam.flat_ema); the discriminators are not averaged.  Parameters are all there is to average: the generators hold no
    buffers (InstanceNorm keeps no running statistics here); the only buffers of any model are the discriminators'
    spectral-norm `weight_u` / `weight_v`."""
    _ema_in_scope = False

    def _ema_optimizer(self):
        opt = getattr(self, "optimizer_G", None)
        if opt is None:
            opt = getattr(self, "optimizer", None)
        return opt if opt is not None and getattr(opt, "ema_decay", None) is not None else None

    @property
    def ema_enabled(self):
        return self._ema_optimizer() is not None

    @contextlib.contextmanager
    def ema_scope(self):
        """The averaged weights in the parameters' place for the duration of the block (evaluation), the raw ones back afterwards,
        also when the block raises.  Does nothing when the model keeps no average.  Not re-entrant."""
        if self._ema_in_scope:
            raise RuntimeError("ema_scope() is already active on this model: it does not nest")
        opt = self._ema_optimizer()
        if opt is None:
            yield self
            return
        opt.swap_ema()
        self._ema_in_scope = True
        try:
            yield self
        finally:
            self._ema_in_scope = False
            opt.swap_ema()

    def _ema_names(self, opt):
        names = {id(p): name for name, p in self.named_parameters()}
        return [names[id(p)] for p in opt.params]

    def ema_state_dict(self):
        """{state_dict key: averaged tensor} of the tracked parameters: state_dict()'s names and OIHW shapes."""
        opt = self._ema_optimizer()
        if opt is None:
            raise RuntimeError("ema_state_dict(): this model keeps no averaged weights (configure_optimizers(ema_decay=...))")
        return dict(zip(self._ema_names(opt), opt.ema_state()["tensors"]))

    def save_ema_state(self):
        """{"decay", "updates", "state_dict": ema_state_dict()} — what a checkpoint stores under `vcg_ema`."""
        sd = self.ema_state_dict()
        opt = self._ema_optimizer()
        return {"decay": opt.ema_decay, "updates": opt.ema_updates, "state_dict": sd}

    def load_ema_state(self, state):
        opt = self._ema_optimizer()
        if opt is None:
            raise RuntimeError("load_ema_state(): this model keeps no averaged weights (configure_optimizers(ema_decay=...))")
        names, sd = self._ema_names(opt), state["state_dict"]
        missing = [n for n in names if n not in sd]
        if missing or len(sd) != len(names):
            extra = sorted(set(sd) - set(names))
            raise KeyError(f"averaged weights do not match the tracked parameters: missing {missing[:3]}, unexpected {extra[:3]} "
                           f"({len(sd)} saved, {len(names)} tracked)")
        opt.load_ema_state({"updates": state["updates"], "tensors": [sd[n] for n in names]})


class _OptimizerStatesMixin(_EmaMixin):
    """The optimizers of a model, by attribute name: one `optimizer`, or `optimizer_G` / `optimizer_D` (_GanMixin)."""
    _opt_names = ("optimizer",)

    def _single_optimizer(self, params, lr, betas, clip_grad_norm, ema_decay, pool_size):
        """configure_optimizers of the models with one Adam and no discriminator."""
        _refuse_pool(self, pool_size)
        self.optimizer = FusedAdam(params, lr=lr, betas=betas, max_grad_norm=_max_grad_norm(clip_grad_norm),
                                   ema_decay=_ema_decay(ema_decay))
        return self.optimizer

    def save_optimizer_states(self):
        out = {}
        for name in self._opt_names:
            opt = getattr(self, name)
            if opt is None:
                raise ValueError("Optimizer has not been configured yet." if len(self._opt_names) == 1
                                 else "Optimizers have not been configured yet.")
            out[name] = opt.state_dict()
        return out

    def load_optimizer_states(self, states):
        for name in self._opt_names:
            if getattr(self, name) is None:
                raise ValueError("Optimizer has not been configured yet." if len(self._opt_names) == 1
                                 else "Optimizers have not been configured yet.")
        for name in self._opt_names:
            if name not in states:
                raise KeyError(f"{name} state not found in states")
            getattr(self, name).load_state_dict(states[name])


class _GanMixin(_PoolMixin, _OptimizerStatesMixin):
    """The models with discriminators (`_discriminators`, trained by optimizer_D) beside their generators (`_generators`,
    optimizer_G): the optimizer pair and the alternating G then D update."""
    _opt_names = ("optimizer_G", "optimizer_D")
    gan_objective = LSGAN                        # configure_loss(gan_objective=..., gan_label_smooth=...) replaces it
    fm_term = None                               # (weight, FeatureMatchingLoss) after configure_loss(lambda_fm > 0, fm_mode=...)

    def _configure_fm(self, kwargs):
        """The discriminator feature-matching term of a GAN model: lambda_fm times, per discriminator, the distance between its
        block activations on the generated batch and on the real one (Losses.FeatureMatchingLoss), the real side a constant.  It
        sits in G_loss alone: the G-phase backward takes the discriminators' data gradient only (`_alternating_step`), the D phase
        differentiates D_loss, so the discriminator update is the one without the term.  With the weight at its default 0
        `fm_term` is None: no loss object exists, and the step computes, launches and reports exactly what it did before.  The
        element-wise mode needs batches whose images correspond, which an unpaired cycle model's do not."""
        lam, mode = _fm_config(kwargs)
        if mode == "pair" and not getattr(self, "paired", True):
            raise ValueError(f"fm_mode='pair': the batches of an unpaired {type(self).__name__} are not aligned image by image; "
                             "use fm_mode='mean', which matches the expected features")
        self.fm_term = None if lam == 0.0 else (lam, FeatureMatchingLoss(mode))

    @property
    def fm_enabled(self):
        return self.fm_term is not None

    def _disc(self, D, image):
        """One discriminator pass -> (block activations or None, logits): the activations only when the term wants them."""
        return D.features(image) if self.fm_term is not None else (None, D(image))

    def _add_fm(self, t, terms, weights, pairs):
        """Appends the term on the (generated, real) activation lists of the step's discriminators to the generator objective's
        (terms, weights) and to the step's scalars `t`; on the main stream, after the direction join."""
        if self.fm_term is not None:
            lam, fn = self.fm_term
            values = [fn(fake, real) for fake, real in pairs]
            t["loss_fm"] = values[0] if len(values) == 1 else ops.weighted_sum(values, [1.0] * len(values))
            terms.append(t["loss_fm"])
            weights.append(lam)

    def _fm_spec(self, spec):
        """`spec` (_report) with loss_fm after the keys the model reports without the term; unchanged with the weight 0."""
        return spec + (_same("loss_fm") if self.fm_term is not None else ())

    def _gan_optimizers(self, lr, betas, clip_grad_norm, ema_decay, pool_size, pool_seed):
        # pool_size > 0: an image history pool of that many images per discriminator (DX pools F(y), DY pools G(x), D pools G(x)),
        # their plans drawn from generators seeded from pool_seed (_PoolMixin)
        self._make_pools(self._discriminators, pool_size, pool_seed)
        # one bound, two norms: the generators' and the discriminators' gradients are clipped each by their own
        bound = _max_grad_norm(clip_grad_norm)
        g_params, d_params = ([p for n in names for p in getattr(self, n).parameters()]
                              for names in (self._generators, self._discriminators))
        self.optimizer_G = FusedAdam(g_params, lr=lr, betas=betas, max_grad_norm=bound,
                                     ema_decay=_ema_decay(ema_decay))            # the generators' average; none for discriminators
        self.optimizer_D = FusedAdam(d_params, lr=lr, betas=betas, max_grad_norm=bound)
        return self.optimizer_G, self.optimizer_D

    def _alternating_step(self, G_loss, D_loss):
        """Both updates from one forward, whose caller zeroed optimizer_G's gradients before it: the G-phase backward takes only
        the discriminators' data gradient, the D-phase backward their weight gradients from the same saved activations."""
        opt_G, opt_D, red = self.optimizer_G, self.optimizer_D, self.grad_reducer
        if red is not None:
            red.begin(opt_G)                     # generator buckets are all-reduced from inside the backward as they complete
        # generator gradients reach the generators only (the discriminators contribute their data gradient)
        with ops.no_wgrad(opt_D.params):
            ops.backward_overlapped(G_loss, inputs=opt_G.params, retain_graph=True)
        if red is not None:
            red.start(opt_G)                     # whatever is left; it runs under the D backward below
        # discriminator gradients from the same activations reach the discriminators only — what detaching G(x), F(y) achieves
        # in the reference (:2028-2029).  Neither this backward nor D_loss reads a generator parameter, so running it before
        # optimizer_G.step() changes nothing.
        opt_D.zero_grad()
        if red is not None:
            red.begin(opt_D)
        with ops.no_dgrad([getattr(self, n).model[0]._spec for n in self._discriminators]):
            ops.backward_overlapped(D_loss, inputs=opt_D.params)
        if red is not None:
            red.start(opt_D)
            red.finish(opt_G)
        opt_G.step()
        if red is not None:
            red.finish(opt_D)
        opt_D.step()


def _same(*names):
    """_report entries reported under their source's own name."""
    return tuple((n, n) for n in names)


_GX, _GX_FY = (("Gx", None),), (("Gx", None), ("Fy", None))      # validation's translated batches (_report's `images`)


def _report(model, t, spec, training, **images):
    """What a step returns.  `spec`: the model's ordered (reported name, source) pairs — a source is a key of the step's device
    scalars `t`, a pair of keys (their sum on the host: total_loss = G_loss + D_loss) or None (the entry of `images`).  All
    sources and, after a training step, what the optimizer steps left on the device (_clip_scalars) cross in ONE device->host
    copy, averaged over ranks when training; the clip keys follow the model's own.  A new step-level metric is added here,
    once."""
    clip = _clip_scalars(**{n[len("optimizer"):]: getattr(model, n) for n in model._opt_names}) if training else {}
    named = {}
    for _, src in spec:
        for s in (src,) if isinstance(src, str) else src or ():
            named[s] = t[s]
    named.update(clip)
    host = _metrics_to_host(named, model.grad_reducer if training else None)
    out = {}
    for name, src in spec:
        out[name] = images[name] if src is None else host[src] if isinstance(src, str) else host[src[0]] + host[src[1]]
    out.update({k: host[k] for k in clip})
    return out


class Autoencoder(_OptimizerStatesMixin, nn.Module):
    """Encoder -> Decoder, L1 loss, one Adam  (reference Networks.py:276-413)."""

    def __init__(self):
        super().__init__()
        self.encoder = Encoder()
        self.decoder = Decoder()
        self.optimizer = None
        self.grad_reducer = None
        self.loss_fn = None
        self.image_terms = ()
        self.apply(self._init_weights)

    def _init_weights(self, module):
        _kaiming_relu_init(module)

    def forward(self, x):
        return self.decoder(self.encoder(x))

    def configure_optimizers(self, lr=1e-4, betas=(0.5, 0.999), decoder_only=False, clip_grad_norm=0.0, ema_decay=0.0, pool_size=0):
        params = self.decoder.parameters() if decoder_only else self.parameters()
        return self._single_optimizer(params, lr, betas, clip_grad_norm, ema_decay, pool_size)

    def configure_loss(self, **kwargs):
        _refuse_swd(self, kwargs)
        _refuse_kl_control(self, kwargs)
        _refuse_gan_objective(self, kwargs)
        _refuse_fm(self, kwargs)
        self.loss_fn = TranslationLoss()
        self.image_terms = _image_terms(kwargs)

    def training_step(self, batch):
        """Written out (no _report): the reference's NaN / Inf guard reads the loss on the host before the update, and the plain
        step reuses that value instead of a second copy."""
        _refuse_training_in_ema_scope(self)
        if self.loss_fn is None:
            raise ValueError("Loss function has not been configured yet.")
        if self.optimizer is None:
            raise ValueError("Optimizer has not been configured yet.")
        x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
        output = self(x)
        loss_trans = self.loss_fn(output, y)
        G_loss = loss_trans
        # (a caller's stand-in for `self` need not know the terms)
        extra, weights = _eval_image_terms(getattr(self, "image_terms", ()), [(output, y)])
        if extra:
            G_loss = ops.weighted_sum([loss_trans, *extra.values()], [1.0, *weights])
        value = float(G_loss.detach())                 # the reference's isnan/isinf guard syncs here too (:357)
        bad = math.isnan(value) or math.isinf(value)
        red = self.grad_reducer
        if red is not None:
            # data parallel: the decision is collective — a rank that skipped alone would never join the gradient
            # exchange the others enter, and the replicas would diverge
            bad = red.any_rank(bad)
        if bad:
            print("NaN or Inf detected in loss during training step; skipping the update.")
            self.optimizer.zero_grad()
            m = {"nan_detected": True, "G_loss": float("nan"), "loss_trans": float("nan"), "total_loss": float("nan")}
            m.update({k: float("nan") for k in extra})
            if getattr(self.optimizer, "clip_state", None) is not None:      # skipped here, on the host, before any gradient existed
                m["grad_norm"], m["grad_skipped"] = float("nan"), 1.0
            return m
        _backward_and_step(G_loss, self.optimizer, red)
        clip = _clip_scalars(**{"": self.optimizer})
        if extra:
            m = _metrics_to_host({"G_loss": G_loss, "loss_trans": loss_trans, **extra, **clip}, red)
            out = {"G_loss": m["G_loss"], "loss_trans": m["loss_trans"], "total_loss": m["G_loss"]}
            out.update({k: m[k] for k in (*extra, *clip)})
            return out
        if red is not None or clip:
            m = _metrics_to_host({"loss_trans": loss_trans, **clip}, red)
            value = m["loss_trans"]                                               # the global-batch mean, as every other model logs
            out = {"G_loss": value, "loss_trans": value, "total_loss": value}
            out.update({k: m[k] for k in clip})
            return out
        return {"G_loss": value, "loss_trans": value, "total_loss": value}

    def validation_step(self, batch):
        if self.loss_fn is None:
            raise ValueError("Loss function has not been configured yet.")
        with torch.no_grad():
            x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
            output = self(x)
            if self.image_terms:
                loss_trans = self.loss_fn(output, y)
                extra, weights = _eval_image_terms(self.image_terms, [(output, y)])
                t = {"G_loss": ops.weighted_sum([loss_trans, *extra.values()], [1.0, *weights]), "loss_trans": loss_trans, **extra}
                return _report(self, t, (("G_loss", "G_loss"), ("total_loss", "G_loss")) + _same("loss_trans", *extra) + _GX,
                               False, Gx=output)
            value = float(self.loss_fn(output, y))
            return {"G_loss": value, "total_loss": value, "loss_trans": value, "Gx": output}


class VariationalAutoencoder(_OptimizerStatesMixin, nn.Module):
    """Encoder -> VAE bottleneck -> Decoder, L1 + lambda_kl * KL  (reference Networks.py:855-988)."""

    def __init__(self, latent_dim=64):
        super().__init__()
        self.encoder = Encoder()
        self.variational_encoder_block = VariationalEncoderBlock(in_channels=1024, latent_dim=latent_dim)
        self.variational_decoder_block = VariationalDecoderBlock(latent_dim=latent_dim, out_channels=1024)
        self.decoder = Decoder()
        self.optimizer = None
        self.grad_reducer = None
        self.loss_trans_fn = None
        self.loss_kl_fn = None
        self.lambda_kl = 0
        self.image_terms = ()
        self.apply(self._init_weights)

    def _init_weights(self, module):
        _kaiming_relu_init(module)

    def forward(self, x):
        encoded = self.encoder(x)
        z, mu, logvar = self.variational_encoder_block(encoded)
        Gx = self.decoder(self.variational_decoder_block(z))
        return Gx, mu, logvar

    def latent(self, x):
        """The encoder half of `forward`: (mu, raw logvar) of x's latent distribution.  Draws no eps."""
        return self.variational_encoder_block.latent(self.encoder(x))

    def decode(self, z):
        """The decoder half of `forward` on latents z (any batch)."""
        return self.decoder(self.variational_decoder_block(z))

    def configure_optimizers(self, lr=1e-4, betas=(0.5, 0.999), clip_grad_norm=0.0, ema_decay=0.0, pool_size=0):
        return self._single_optimizer(self.parameters(), lr, betas, clip_grad_norm, ema_decay, pool_size)

    def configure_loss(self, **kwargs):
        _refuse_swd(self, kwargs)
        _refuse_gan_objective(self, kwargs)
        _refuse_fm(self, kwargs)
        self.loss_trans_fn = TranslationLoss()
        self.loss_kl_fn = _configure_kl(self, kwargs)
        self.image_terms = _image_terms(kwargs)

    def _check_configured(self):
        if self.optimizer is None:
            raise ValueError("Optimizer has not been configured yet.")
        if self.loss_trans_fn is None:
            raise ValueError("Translation loss function has not been configured yet.")
        if self.loss_kl_fn is None:
            raise ValueError("KL divergence loss function has not been configured yet.")

    def _losses(self, batch, training=False):
        """-> (G(x), the step's scalars in the order they are reported: G_loss, loss_trans, loss_kl, [loss_kl_fb, kl_active],
        [loss_ssim], [loss_grad], [loss_freq], [loss_msssim])"""
        x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
        output, mu, logvar = self(x)
        loss_trans = self.loss_trans_fn(output, y)
        kl, kl_objective, _ = _kl_terms(self.loss_kl_fn, [(mu, logvar)])
        extra, weights = _eval_image_terms(self.image_terms, [(output, y)])
        named = {"G_loss": None, "loss_trans": loss_trans, **kl, **extra}
        named["G_loss"] = ops.weighted_sum([loss_trans, kl_objective, *extra.values()], [1.0, _kl_weight(self, training), *weights])
        return output, named

    def _spec(self, named, training):
        return _kl_keys(self, _same(*(k for k in named if k not in ("loss_kl_fb", "kl_active"))), training)

    def training_step(self, batch):
        _refuse_training_in_ema_scope(self)
        self._check_configured()
        _, named = self._losses(batch, True)
        _backward_and_step(named["G_loss"], self.optimizer, self.grad_reducer)
        return _report(self, named, self._spec(named, True), True, **_kl_host(self, True))

    def validation_step(self, batch):
        self._check_configured()
        with torch.no_grad():
            output, named = self._losses(batch)
            return _report(self, named, self._spec(named, False) + _GX, False, Gx=output)


# --------------------------------------------------------------------------- the two translation directions
def _vae_pair(vae_a, a, ticket_a, vae_b, b, ticket_b, fork):
    """vae_a(a) on the caller's stream and vae_b(b) on `fork`'s second stream, issued alternately in half-generator pieces
    (encoder | bottleneck + decoder): the second stream has work after a quarter of the host time a whole generator takes to
    issue, and — autograd replays in reverse issue order — the backward alternates between the two chains at the same
    granularity instead of one whole generator at a time (against whole generators alternating between the streams, three
    alternations: CycleVAEGAN step 32.54 / 32.64 / 34.36 -> 31.89 / 31.98 / 33.41 ms; block by block, through generator
    coroutines, measured no better: 32.4 vs 32.3)."""
    def tail(vae, enc, ticket):                  # VariationalAutoencoder.forward after its encoder
        with ops.use_ticket(ticket):
            z, mu, lv = vae.variational_encoder_block(enc)
        return vae.decoder(vae.variational_decoder_block(z)), mu, lv

    ea = vae_a.encoder(a)
    with fork.second():
        eb = vae_b.encoder(b)
    ra = tail(vae_a, ea, ticket_a)
    with fork.second():
        rb = tail(vae_b, eb, ticket_b)
    return ra, rb


def _ae_pair(ae_a, a, ae_b, b, fork):
    """The same for two plain autoencoders."""
    ea = ae_a.encoder(a)
    with fork.second():
        eb = ae_b.encoder(b)
    ra = ae_a.decoder(ea)
    with fork.second():
        rb = ae_b.decoder(eb)
    return ra, rb


def _fork(x, y):
    """Open the second stream for a step over `x` and `y` (ops.DirectionFork; the caller joins it).  Both inputs' magnitudes are
    published first: a tensor that two streams will read must not be measured by one of them after they have forked."""
    ops.premeasure(x)
    ops.premeasure(y)
    return ops.DirectionFork(x.device)


def _eps_shape(vae, x):
    """Shape of the eps one forward of `vae` on `x` draws."""
    n, _, h, w = x.shape
    return (n, vae.variational_encoder_block.latent_dim, h // 16, w // 16)


def _two_directions(G, F, x, y, fork=None, tickets=None, identity=None):
    """x -> G -> F and y -> F -> G for two autoencoders or two VAEs -> ((G(x), F(G(x)), F(y), G(F(y))), their (mu, logvar)s
    flattened in that order — empty for autoencoders —, G(y), F(x)).

    With a `fork`: x -> G -> F on the caller's stream and y -> F -> G on the second one, issued interleaved (_vae_pair) so that
    both have work from the start.  Same results bit for bit: VAEs draw at `tickets`, the positions of those four calls reserved
    in the reference's call order.  Without: the four calls in the reference's order on one stream; `identity(generator,
    image)`, if given, is called for G(y) after G(x) and for F(x) after F(y) — where the reference's CycleVAEGAN computes (and
    draws eps for) the identity passes — and G(y), F(x) are what it returns (None otherwise)."""
    Gy = Fx = None
    if fork is None:
        rGx = G(x)
        if identity is not None:
            Gy = identity(G, y)
        rFGx = F(rGx[0] if isinstance(rGx, tuple) else rGx)
        rFy = F(y)
        if identity is not None:
            Fx = identity(F, x)
        rGFy = G(rFy[0] if isinstance(rFy, tuple) else rFy)
    elif tickets is None:
        rGx, rFy = _ae_pair(G, x, F, y, fork)
        rFGx, rGFy = _ae_pair(F, rGx, G, rFy, fork)
    else:
        rGx, rFy = _vae_pair(G, x, tickets[0], F, y, tickets[2], fork)
        rFGx, rGFy = _vae_pair(F, rGx[0], tickets[1], G, rFy[0], tickets[3], fork)
    rs = (rGx, rFGx, rFy, rGFy)
    if isinstance(rGx, tuple):                   # VariationalAutoencoder.forward: (image, mu, logvar)
        return tuple(r[0] for r in rs), tuple(s for r in rs for s in r[1:]), Gy, Fx
    return rs, (), Gy, Fx


def _discriminate(DY, DX, Gx, Fy, x, y, fork=None, run=None):
    """-> DY(G(x)), DX(F(y)), DX(x), DY(y), issued DY(G(x)), DX(F(y)), DY(y), DX(x): alternately on the two streams of `fork`
    (32.64 -> 32.42 ms over three A/B pairs), each discriminator seeing its fake before its real batch as in the reference
    (spectral norm's power iteration advances per call).  `run(D, image)`, if given, stands for D(image) (_GanMixin._disc: each
    result is then an (activations, logits) pair)."""
    second = fork.second if fork is not None else contextlib.nullcontext
    if run is None:
        run = lambda D, image: D(image)          # noqa: E731
    DYGx = run(DY, Gx)
    with second():
        DXFy = run(DX, Fy)
    DYy = run(DY, y)
    with second():
        DXx = run(DX, x)
    return DYGx, DXFy, DXx, DYy


class CycleVAEGAN(_SwdMixin, _GanMixin, nn.Module):
    """Two VAEs (G: X->Y, F: Y->X) + two discriminators; cycle + LSGAN + KL (+identity if paired);
    alternating G then D update  (reference Networks.py:1872-2150).

    Differences from the reference are work that cannot change any result:
      * unpaired mode does not compute G(y), F(x) inside training_step (their outputs feed only
        the identity loss, reference :2016-2018); their eps draws are still consumed;
      * the discriminators run ONCE per step: the G-phase backward takes only the data gradient
        and the D-phase backward takes the weight gradients from the same saved activations
        (the reference recomputes four D forwards at :2032-2035 with unchanged D weights, and
        discards the D weight gradients of its G-phase backward at :2025).
    """
    _generators, _discriminators = ("F", "G"), ("DX", "DY")
    _variational = True                          # CycleAEGAN: plain autoencoders — no eps, no KL term
    _GAN_G_TERMS = ("loss_gan_g_x_fake", "loss_gan_g_y_fake")        # what G_loss takes of the LSGAN generator loss

    def __init__(self, latent_dim=64, paired=True):
        super().__init__()
        self.F = self._make_generator(latent_dim)
        self.G = self._make_generator(latent_dim)
        self.DX = Discriminator()
        self.DY = Discriminator()
        self.paired = paired
        self.apply(self._init_weights)
        self.debug_mode = False
        self.debug_info = {}
        self.optimizer_G = None
        self.optimizer_D = None
        self.loss_cycle = None
        self.loss_gan_gen = None
        self.loss_gan_disc = None
        self.loss_identity = None
        self.loss_kl = None
        self.image_terms = ()
        # data-parallel hook: set by parallel.attach(); called as reducer(phase, optimizer)
        self.grad_reducer = None

    def _make_generator(self, latent_dim):
        return VariationalAutoencoder(latent_dim)

    def _init_weights(self, module):
        _kaiming_relu_init(module)

    def enable_debug_mode(self, enabled=True):
        self.debug_mode = enabled

    def forward(self, x, y):
        x, y = ops.to_nhwc(x), ops.to_nhwc(y)
        Gx, mu_x, logvar_x = self.G(x)
        Gy, _, _ = self.G(y)
        FGx, mu_FGx, logvar_FGx = self.F(Gx)
        Fy, mu_y, logvar_y = self.F(y)
        Fx, _, _ = self.F(x)
        GFy, mu_GFy, logvar_GFy = self.G(Fy)
        DYGx = self.DY(Gx)
        DXFy = self.DX(Fy)
        DXx = self.DX(x)
        DYy = self.DY(y)
        return (Gx, FGx, Fy, GFy, mu_x, logvar_x, mu_FGx, logvar_FGx, mu_y, logvar_y, mu_GFy, logvar_GFy,
                DYGx, DXFy, DXx, DYy, Gy, Fx)

    def configure_optimizers(self, lr=1e-4, betas=(0.5, 0.999), clip_grad_norm=0.0, ema_decay=0.0, pool_size=0, pool_seed=0):
        return self._gan_optimizers(lr, betas, clip_grad_norm, ema_decay, pool_size, pool_seed)

    def configure_loss(self, **kwargs):
        self.loss_cycle = CycleConsistencyLoss()
        self.loss_gan_gen, self.loss_gan_disc = _configure_gan(self, kwargs)
        if self.paired:
            self.loss_identity = IdentityLoss()
        if self._variational:
            self.loss_kl = _configure_kl(self, kwargs)
        else:
            _refuse_kl_control(self, kwargs)
        self.lambda_gan = kwargs.get("lambda_gan", 1.0)
        self.lambda_identity = kwargs.get("lambda_identity", 5.0)
        self.lambda_cycle = kwargs.get("lambda_cycle", 10.0)
        self.image_terms = _image_terms(kwargs)
        self._configure_swd(kwargs)
        self._configure_fm(kwargs)

    def _check_configured(self, need_opt=True):
        if (self.loss_cycle is None or self.loss_gan_gen is None or self.loss_gan_disc is None
                or (self._variational and self.loss_kl is None)):
            raise ValueError("Loss functions have not been configured yet.")
        if self.paired and self.loss_identity is None:
            raise ValueError("Identity loss not configured for paired mode.")
        if need_opt and (self.optimizer_G is None or self.optimizer_D is None):
            raise ValueError("Optimizers have not been configured yet.")

    def _skip_vae(self, ref_shape_src, vae):
        """Advance the eps stream past a VAE forward that is not computed."""
        ops.next_eps(_eps_shape(vae, ref_shape_src), ref_shape_src.device, skip=True)

    def _identity_pass(self, vae, image):
        """G(y) / F(x) at their place in the reference's call order: they feed only the identity loss, so unpaired they are not
        computed and only their eps draw is consumed."""
        if self.paired:
            return vae(image)[0]
        self._skip_vae(image, vae)

    def _generator_losses(self, x, y, two_streams=False, training=False):
        """Forward of both generators and everything G_loss needs (reference :1997-2018, CycleAEGAN :1733-1753).  `two_streams`
        (training_step asks for it when the weight gradients overlap too): the unpaired forward with x -> G -> F -> DY on the
        caller's stream and y -> F -> G -> DX on a second one (_two_directions); the eps draws are reserved in the reference's
        call order G(x), [G(y)], F(G(x)), F(y), [F(x)], G(F(y))."""
        fork = tickets = None
        if two_streams and not self.paired and x.is_cuda:
            if self._variational:
                shp = _eps_shape(self.G, x)
                tk = ops.eps_tickets([(shp, False), (shp, True), (shp, False), (shp, False), (shp, True), (shp, False)], x.device)
                tickets = (tk[0], tk[2], tk[3], tk[5])
            fork = _fork(x, y)
        (Gx, FGx, Fy, GFy), stats, Gy, Fx = _two_directions(self.G, self.F, x, y, fork, tickets,
                                                             self._identity_pass if self._variational else None)
        (aDYGx, DYGx), (aDXFy, DXFy), (aDXx, DXx), (aDYy, DYy) = _discriminate(self.DY, self.DX, Gx, Fy, x, y, fork, self._disc)
        if fork is not None:
            fork.join()

        t = {}
        t["loss_cycle"] = self.loss_cycle(x, y, FGx, GFy)
        gan_x, gan_y = _GanTerms(self.gan_objective, DXx, DXFy), _GanTerms(self.gan_objective, DYy, DYGx)
        t["loss_gan_g_x_fake"], t["d_x_fake_mean"] = gan_x.g_fake()
        t["loss_gan_g_y_fake"], t["d_y_fake_mean"] = gan_y.g_fake()
        t["loss_gan_g_x_real"], t["d_x_real_mean"] = gan_x.g_real()
        t["loss_gan_g_y_real"], t["d_y_real_mean"] = gan_y.g_real()
        t["loss_gan_g"] = ops.weighted_sum([t[k] for k in self._GAN_G_TERMS], [1.0] * len(self._GAN_G_TERMS))
        terms, weights = [t["loss_cycle"], t["loss_gan_g"]], [self.lambda_cycle, self.lambda_gan]
        if self._variational:
            kl, kl_objective, _ = _kl_terms(self.loss_kl, [(stats[2 * i], stats[2 * i + 1]) for i in range(4)])
            t.update(kl)
            terms.append(kl_objective)
            weights.append(_kl_weight(self, training))
        if self.paired:
            if not self._variational:            # CycleAEGAN's identity passes follow the discriminators (reference :1749-1751)
                Fx, Gy = self.F(x), self.G(y)
            t["loss_identity"] = self.loss_identity(x, y, Fx, Gy)
            terms.append(t["loss_identity"])
            weights.append(self.lambda_identity)
        # the optional cycle terms, each on the L1 cycle term's operands; FGx and GFy are joined by now, as for loss_cycle
        extra, extra_weights = _eval_image_terms(self.image_terms, [(FGx, x), (GFy, y)])
        t.update(extra)
        terms, weights = terms + list(extra.values()), weights + extra_weights
        self._add_swd(t, terms, weights, Gx, Fy, x, y)     # the translated batches against the other domain's: needs no pairing
        # fm(DY: G(x) against y) + fm(DX: F(y) against x), on the shared discriminator passes; both streams are joined by now
        self._add_fm(t, terms, weights, [(aDYGx, aDYy), (aDXFy, aDXx)])
        t["G_loss"] = ops.weighted_sum(terms, weights)
        # discriminator objective on the SAME discriminator outputs (reference :2038-2040)
        t["D_loss_x_real"], _ = gan_x.d_real()
        t["D_loss_x_fake"], _ = gan_x.d_fake()
        t["D_loss_y_real"], _ = gan_y.d_real()
        t["D_loss_y_fake"], _ = gan_y.d_fake()
        t["D_loss"] = ops.weighted_sum([t["D_loss_x_real"], t["D_loss_x_fake"], t["D_loss_y_real"], t["D_loss_y_fake"]],
                                       [1.0] * 4)
        return t, Gx, Fy

    _METRIC_KEYS = ("G_loss", "D_loss", "D_loss_x_real", "D_loss_x_fake", "D_loss_y_real", "D_loss_y_fake",
                    "loss_cycle", "loss_gan_g", "loss_gan_g_x_real", "loss_gan_g_x_fake", "loss_gan_g_y_real",
                    "loss_gan_g_y_fake", "loss_kl")
    _MEAN_KEYS = ("d_x_real_mean", "d_x_fake_mean", "d_y_real_mean", "d_y_fake_mean")

    def _report_spec(self, training):
        keys = self._METRIC_KEYS + (self._MEAN_KEYS if training else ())
        if self.paired:
            keys += ("loss_identity",)
        keys += tuple(name for name, _, _ in self.image_terms)
        return self._fm_spec(_kl_keys(self, (("total_loss", ("G_loss", "D_loss")),) + _same(*keys) + self._swd_spec()
                                      + (() if training else _GX_FY), training))

    def _pooled_d_terms(self, t, Gx, Fy):
        """The discriminators' fake terms with image history pools (_PoolMixin), after the forward (both direction streams are
        joined by then) on the main stream.  Replaces D_loss_x_fake / D_loss_y_fake and D_loss in `t` for the discriminators whose
        batch was exchanged; G_loss and everything the G phase differentiates stay the shared pass's."""
        fake_x, fake_y = Fy.detach(), Gx.detach()
        shown_x, extra_x = self._shown_to("DX", fake_x)
        shown_y, extra_y = self._shown_to("DY", fake_y)
        if extra_x:
            t["D_loss_x_fake"], _ = _GanTerms(self.gan_objective, None, self.DX(shown_x)).d_fake()
        if extra_y:
            t["D_loss_y_fake"], _ = _GanTerms(self.gan_objective, None, self.DY(shown_y)).d_fake()
        if extra_x or extra_y:
            t["D_loss"] = ops.weighted_sum([t["D_loss_x_real"], t["D_loss_x_fake"], t["D_loss_y_real"], t["D_loss_y_fake"]],
                                           [1.0] * 4)
        if self.debug_mode:
            self._debug_store().update(fake_x=fake_x, fake_y=fake_y, d_fake_x=shown_x, d_fake_y=shown_y)

    def training_step(self, batch):
        _refuse_training_in_ema_scope(self)
        self._check_configured()
        x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
        self.optimizer_G.zero_grad()
        t, Gx, Fy = self._generator_losses(x, y, two_streams=ops.two_directions(), training=True)
        if self.image_pools:
            self._pooled_d_terms(t, Gx, Fy)
        self._alternating_step(t["G_loss"], t["D_loss"])
        return _report(self, t, self._report_spec(True), True, **_kl_host(self, True))

    def validation_step(self, batch):
        self._check_configured(need_opt=False)
        with torch.no_grad():
            x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
            t, Gx, Fy = self._generator_losses(x, y)
            return _report(self, t, self._report_spec(False), False, Gx=Gx.detach(), Fy=Fy.detach())


class CycleAEGAN(CycleVAEGAN):
    """Two plain autoencoders (G: X->Y, F: Y->X) + two discriminators; cycle + LSGAN (+identity if paired), alternating
    G then D update  (reference Networks.py:1618-1869).  CycleVAEGAN's wiring minus the VAE block: no KL term and no
    eps draws, `forward` returns 10 tensors, and the generator objective carries the WHOLE LSGAN generator loss
    (`loss_gan_g = loss_gan_g_x + loss_gan_g_y`, real + fake terms, :1745-1748) where CycleVAEGAN takes only the fake
    terms — the real terms have no gradient into F and G, but they are part of `G_loss` and of the `loss_gan_g` metric.
    The step itself (one discriminator pass serving both phases, exchange hooks, side stream) is CycleVAEGAN's."""
    _variational = False
    _GAN_G_TERMS = ("loss_gan_g_x_real", "loss_gan_g_x_fake", "loss_gan_g_y_real", "loss_gan_g_y_fake")
    _METRIC_KEYS = tuple(k for k in CycleVAEGAN._METRIC_KEYS if k != "loss_kl")

    def __init__(self, paired=True):
        super().__init__(paired=paired)

    def _make_generator(self, latent_dim):
        return Autoencoder()

    def forward(self, x, y):
        x, y = ops.to_nhwc(x), ops.to_nhwc(y)
        Gx = self.G(x)
        Gy = self.G(y)
        FGx = self.F(Gx)
        Fy = self.F(y)
        Fx = self.F(x)
        GFy = self.G(Fy)
        return Gx, FGx, Fy, GFy, self.DY(Gx), self.DX(Fy), self.DX(x), self.DY(y), Gy, Fx


class _CycleNoGAN(_SwdMixin, _OptimizerStatesMixin, nn.Module):
    """Two generators G: X->Y, F: Y->X trained on the cycle loss alone (+ KL for VAEs, + translation loss when paired),
    one Adam over both — the shared body of CycleAE and CycleVAE (reference Networks.py:1350-1616)."""

    def _init_common(self, paired):
        self.paired = paired
        self.optimizer = None        # (CycleVAE.__init__ in the reference leaves this attribute unset until configured)
        self.grad_reducer = None
        self.loss_cycle = None
        self.loss_trans = None
        self.loss_kl = None
        self.lambda_cycle = 0
        self.lambda_kl = 0

    def forward(self, x, y):
        return self._fwd(x, y, False)

    def _fwd(self, x, y, two_streams):
        """-> Gx, FGx, Fy, GFy, then for VAEs mu_x, logvar_x, mu_FGx, logvar_FGx, mu_y, logvar_y, mu_GFy, logvar_GFy; eps is drawn
        in the order G(x), F(G(x)), F(y), G(F(y)) (:1489-1494) — on two streams (_two_directions) from tickets reserved so."""
        x, y = ops.to_nhwc(x), ops.to_nhwc(y)
        fork = tickets = None
        if two_streams and x.is_cuda:
            if self._variational:
                tickets = ops.eps_tickets([(_eps_shape(self.G, x), False)] * 4, x.device)
            fork = _fork(x, y)
        images, stats, _, _ = _two_directions(self.G, self.F, x, y, fork, tickets)
        if fork is not None:
            fork.join()
        return images + stats

    def configure_optimizers(self, lr=1e-4, betas=(0.5, 0.999), clip_grad_norm=0.0, ema_decay=0.0, pool_size=0):
        return self._single_optimizer(self.parameters(), lr, betas, clip_grad_norm, ema_decay, pool_size)

    def _check_configured(self, need_opt=True):
        if self.loss_cycle is None or (self._variational and self.loss_kl is None):
            raise ValueError("Loss functions have not been configured yet.")
        if self.paired and self.loss_trans is None:
            raise ValueError("Translation loss not configured for paired mode.")
        if need_opt and self.optimizer is None:
            raise ValueError("Optimizer has not been configured yet.")

    def _losses(self, batch, training=False):
        x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
        fw = self._fwd(x, y, ops.two_directions())     # (a bare model(x, y) stays on one stream: its caller may use a plain backward)
        Gx, FGx, Fy, GFy = fw[:4]
        t = {"loss_cycle": self.loss_cycle(x, y, FGx, GFy)}
        terms, weights = [t["loss_cycle"]], [self.lambda_cycle]
        if self._variational:
            kl, kl_objective, _ = _kl_terms(self.loss_kl, [(fw[4 + 2 * i], fw[5 + 2 * i]) for i in range(4)])
            t.update(kl)
            terms.append(kl_objective)
            weights.append(_kl_weight(self, training))
        if self.paired:
            t["loss_trans"] = ops.weighted_sum([self.loss_trans(Gx, y), self.loss_trans(Fy, x)], [1.0, 1.0])
            terms.append(t["loss_trans"])
            weights.append(1.0)
        self._add_swd(t, terms, weights, Gx, Fy, x, y)     # unpaired, the one term that ties G(x) to domain Y (G = F = identity
        t["G_loss"] = ops.weighted_sum(terms, weights)     # satisfies the cycle loss exactly)
        return t, Gx, Fy

    def _report_spec(self, training):
        """the reference's key order (:1421-1433, :1547-1561): total_loss, loss_cycle, [loss_kl], G_loss, [Gx, Fy], [loss_trans],
        then [loss_swd]"""
        return _kl_keys(self, (("total_loss", "G_loss"),) + _same("loss_cycle", *(("loss_kl",) if self._variational else ()), "G_loss")
                        + (() if training else _GX_FY) + (_same("loss_trans") if self.paired else ()) + self._swd_spec(), training)

    def training_step(self, batch):
        _refuse_training_in_ema_scope(self)
        self._check_configured()
        t, _, _ = self._losses(batch, True)
        _backward_and_step(t["G_loss"], self.optimizer, self.grad_reducer)
        return _report(self, t, self._report_spec(True), True, **_kl_host(self, True))

    def validation_step(self, batch):
        self._check_configured(need_opt=False)
        with torch.no_grad():
            t, Gx, Fy = self._losses(batch)
            return _report(self, t, self._report_spec(False), False, Gx=Gx.detach(), Fy=Fy.detach())


class CycleAE(_CycleNoGAN):
    """reference Networks.py:1350-1480: cycle loss over two plain autoencoders (+ L1(G(x), y) + L1(F(y), x) when paired)."""
    _variational = False

    def __init__(self, paired=True):
        super().__init__()
        self.F = Autoencoder()
        self.G = Autoencoder()
        self._init_common(paired)

    def configure_loss(self, **kwargs):
        _refuse_gan_objective(self, kwargs)
        _refuse_fm(self, kwargs)
        self.loss_cycle = CycleConsistencyLoss()
        if self.paired:
            self.loss_trans = TranslationLoss()
        self.lambda_cycle = kwargs.get("lambda_cycle", 10.0)
        self._configure_swd(kwargs)
        _refuse_kl_control(self, kwargs)


class CycleVAE(_CycleNoGAN):
    """reference Networks.py:1482-1616: the same over two VAEs, plus the four KL terms; eps is drawn in the order
    G(x), F(G(x)), F(y), G(F(y)) (:1489-1494)."""
    _variational = True

    def __init__(self, latent_dim=64, paired=True):
        super().__init__()
        self.F = VariationalAutoencoder(latent_dim)
        self.G = VariationalAutoencoder(latent_dim)
        self._init_common(paired)

    def configure_loss(self, **kwargs):
        _refuse_gan_objective(self, kwargs)
        _refuse_fm(self, kwargs)
        self.loss_cycle = CycleConsistencyLoss()
        if self.paired:
            self.loss_trans = TranslationLoss()
        self.loss_kl = _configure_kl(self, kwargs)
        self.lambda_cycle = kwargs.get("lambda_cycle", 10.0)
        self._configure_swd(kwargs)


class _DoubleStep(_OptimizerStatesMixin, nn.Module):
    """The step of the two pretraining models: one shared encoder, a decoder per modality, one Adam over everything."""

    def forward(self, x, y):
        return self._fwd(x, y, False)

    def configure_optimizers(self, lr=1e-4, betas=(0.5, 0.999), clip_grad_norm=0.0, ema_decay=0.0, pool_size=0):
        return self._single_optimizer(self.parameters(), lr, betas, clip_grad_norm, ema_decay, pool_size)

    def training_step(self, batch):
        _refuse_training_in_ema_scope(self)
        self._check_configured()
        t, _, _ = self._losses(batch, True)
        _backward_and_step(t["G_loss"], self.optimizer, self.grad_reducer)
        return _report(self, t, _kl_keys(self, self._TRAIN, True), True, **_kl_host(self, True))

    def validation_step(self, batch):
        """Gx / Fy are the translations: the encoder runs four times, and a VAE draws eps for each."""
        self._check_configured(need_opt=False)
        with torch.no_grad():
            t, x, y = self._losses(batch)
            return _report(self, t, _kl_keys(self, self._VALIDATION, False), False, Gx=self.translate_A_to_B(x),
                           Fy=self.translate_B_to_A(y))


class DoubleAutoencoder(_DoubleStep):
    """One shared encoder, decoder_A reconstructs the source and decoder_B the target modality — the pretraining model
    for CycleAE (reference Networks.py:415-606).  The encoder runs twice per step, so its weight gradients accumulate
    from both uses (the backward kernels add into the flat gradient buffer)."""
    _TRAIN = _same("G_loss", "loss_recon_A", "loss_recon_B") + (("total_loss", "G_loss"),)
    _VALIDATION = (("G_loss", "G_loss"), ("total_loss", "G_loss")) + _same("loss_recon_A", "loss_recon_B") + _GX_FY

    def __init__(self):
        super().__init__()
        self.encoder = Encoder()
        self.decoder_A = Decoder()
        self.decoder_B = Decoder()
        self.optimizer = None
        self.grad_reducer = None
        self.loss_fn = None

    def _fwd(self, x, y, two_streams):
        x, y = ops.to_nhwc(x), ops.to_nhwc(y)
        if two_streams and x.is_cuda:            # the two modalities on two streams (the shared encoder's gradients meet on the
            fork = _fork(x, y)                   # one weight-gradient stream)
            a = self.decoder_A(self.encoder(x))
            with fork.second():
                b = self.decoder_B(self.encoder(y))
            fork.join()
            return a, b
        return self.decoder_A(self.encoder(x)), self.decoder_B(self.encoder(y))

    def translate_A_to_B(self, x):
        return self.decoder_B(self.encoder(ops.to_nhwc(x)))

    def translate_B_to_A(self, y):
        return self.decoder_A(self.encoder(ops.to_nhwc(y)))

    def create_cycle_ae(self):
        """reference :580-606: G (A->B) = encoder + decoder_B, F (B->A) = encoder + decoder_A."""
        cycle_ae = CycleAE().to(next(self.parameters()).device)
        cycle_ae.G.encoder.load_state_dict(self.encoder.state_dict())
        cycle_ae.G.decoder.load_state_dict(self.decoder_B.state_dict())
        cycle_ae.F.encoder.load_state_dict(self.encoder.state_dict())
        cycle_ae.F.decoder.load_state_dict(self.decoder_A.state_dict())
        return cycle_ae

    def configure_loss(self, **kwargs):
        _refuse_swd(self, kwargs)
        _refuse_kl_control(self, kwargs)
        _refuse_gan_objective(self, kwargs)
        _refuse_fm(self, kwargs)
        self.loss_fn = TranslationLoss()

    def _check_configured(self, need_opt=True):
        if self.loss_fn is None:
            raise ValueError("Loss function has not been configured yet.")
        if need_opt and self.optimizer is None:
            raise ValueError("Optimizer has not been configured yet.")

    def _losses(self, batch, training=False):
        x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
        Gx, Gy = self._fwd(x, y, ops.two_directions())
        t = {"loss_recon_A": self.loss_fn(Gx, x), "loss_recon_B": self.loss_fn(Gy, y)}
        t["G_loss"] = ops.weighted_sum([t["loss_recon_A"], t["loss_recon_B"]], [1.0, 1.0])
        return t, x, y


def _side(side):
    if side not in ("A", "B"):
        raise ValueError(f"side must be 'A' or 'B', got {side!r}")
    return side


class DoubleVariationalAutoencoder(_DoubleStep):
    """Shared encoder, one VAE bottleneck and one decoder per modality — the pretraining model for CycleVAE / CycleVAEGAN
    (reference Networks.py:608-852).  eps draws per forward: block A on enc(x), then block B on enc(y); validation adds one
    per translation."""
    _TRAIN = _same("G_loss", "loss_recon_A", "loss_recon_B", "loss_kl", "loss_kl_A", "loss_kl_B") + (("total_loss", "G_loss"),)
    _VALIDATION = ((("G_loss", "G_loss"), ("total_loss", "G_loss"))
                   + _same("loss_recon_A", "loss_recon_B", "loss_kl", "loss_kl_A", "loss_kl_B") + _GX_FY)

    def __init__(self, latent_dim=64):
        super().__init__()
        self.encoder = Encoder()
        self.vae_encoder_block_A = VariationalEncoderBlock(in_channels=1024, latent_dim=latent_dim)
        self.vae_encoder_block_B = VariationalEncoderBlock(in_channels=1024, latent_dim=latent_dim)
        self.vae_decoder_block_A = VariationalDecoderBlock(latent_dim=latent_dim, out_channels=1024)
        self.vae_decoder_block_B = VariationalDecoderBlock(latent_dim=latent_dim, out_channels=1024)
        self.decoder_A = Decoder()
        self.decoder_B = Decoder()
        self.optimizer = None
        self.grad_reducer = None
        self.loss_trans_fn = None
        self.loss_kl_fn = None
        self.lambda_kl = 0
        self.apply(self._init_weights)

    def _init_weights(self, module):
        _kaiming_relu_init(module)

    def _fwd(self, x, y, two_streams):
        x, y = ops.to_nhwc(x), ops.to_nhwc(y)
        if two_streams and x.is_cuda:            # the two modalities on two streams; eps: block A's draw, then block B's
            n, _, h, w = x.shape
            shp = (n, self.vae_encoder_block_A.latent_dim, h // 16, w // 16)
            tk = ops.eps_tickets([(shp, False)] * 2, x.device)
            fork = _fork(x, y)
            with ops.use_ticket(tk[0]):
                z_x, mu_x, logvar_x = self.vae_encoder_block_A(self.encoder(x))
            Gx = self.decoder_A(self.vae_decoder_block_A(z_x))
            with fork.second():
                with ops.use_ticket(tk[1]):
                    z_y, mu_y, logvar_y = self.vae_encoder_block_B(self.encoder(y))
                Gy = self.decoder_B(self.vae_decoder_block_B(z_y))
            fork.join()
            return Gx, Gy, mu_x, logvar_x, mu_y, logvar_y
        encoded_x = self.encoder(x)
        encoded_y = self.encoder(y)
        z_x, mu_x, logvar_x = self.vae_encoder_block_A(encoded_x)
        z_y, mu_y, logvar_y = self.vae_encoder_block_B(encoded_y)
        Gx = self.decoder_A(self.vae_decoder_block_A(z_x))
        Gy = self.decoder_B(self.vae_decoder_block_B(z_y))
        return Gx, Gy, mu_x, logvar_x, mu_y, logvar_y

    def translate_A_to_B(self, x):
        z, _, _ = self.vae_encoder_block_B(self.encoder(ops.to_nhwc(x)))
        return self.decoder_B(self.vae_decoder_block_B(z))

    def translate_B_to_A(self, y):
        z, _, _ = self.vae_encoder_block_A(self.encoder(ops.to_nhwc(y)))
        return self.decoder_A(self.vae_decoder_block_A(z))

    def latent(self, x, side):
        """(mu, raw logvar) of the bottleneck a translation INTO modality `side` ("A" or "B") samples: translate_A_to_B reads block
        B, translate_B_to_A block A.  Draws no eps."""
        return getattr(self, "vae_encoder_block_" + _side(side)).latent(self.encoder(ops.to_nhwc(x)))

    def decode(self, z, side):
        """Latents z through the decoder block and decoder of modality `side`."""
        side = _side(side)
        return getattr(self, "decoder_" + side)(getattr(self, "vae_decoder_block_" + side)(z))

    def create_cycle_vae(self):
        """reference :701-736: G = encoder + VAE blocks B + decoder_B, F = encoder + VAE blocks A + decoder_A."""
        cycle_vae = CycleVAE(latent_dim=self.vae_encoder_block_A.latent_dim).to(next(self.parameters()).device)
        for gen, sfx in ((cycle_vae.G, "B"), (cycle_vae.F, "A")):
            gen.encoder.load_state_dict(self.encoder.state_dict())
            gen.variational_encoder_block.load_state_dict(getattr(self, "vae_encoder_block_" + sfx).state_dict())
            gen.variational_decoder_block.load_state_dict(getattr(self, "vae_decoder_block_" + sfx).state_dict())
            gen.decoder.load_state_dict(getattr(self, "decoder_" + sfx).state_dict())
        return cycle_vae

    def configure_loss(self, **kwargs):
        _refuse_swd(self, kwargs)
        _refuse_gan_objective(self, kwargs)
        _refuse_fm(self, kwargs)
        self.loss_trans_fn = TranslationLoss()
        self.loss_kl_fn = _configure_kl(self, kwargs)

    def _check_configured(self, need_opt=True):
        if self.loss_trans_fn is None or self.loss_kl_fn is None:
            raise ValueError("Loss functions have not been configured yet.")
        if need_opt and self.optimizer is None:
            raise ValueError("Optimizer has not been configured yet.")

    def _losses(self, batch, training=False):
        x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
        Gx, Gy, mu_x, logvar_x, mu_y, logvar_y = self._fwd(x, y, ops.two_directions())
        t = {"loss_recon_A": self.loss_trans_fn(Gx, x), "loss_recon_B": self.loss_trans_fn(Gy, y)}
        kl, kl_objective, (t["loss_kl_A"], t["loss_kl_B"]) = _kl_terms(self.loss_kl_fn, [(mu_x, logvar_x), (mu_y, logvar_y)])
        t.update(kl)                             # loss_kl_A / loss_kl_B stay each side's plain KL under a floor, as loss_kl does
        t["G_loss"] = ops.weighted_sum([t["loss_recon_A"], t["loss_recon_B"], kl_objective], [1.0, 1.0, _kl_weight(self, training)])
        return t, x, y


class _SingleGAN(_GanMixin, nn.Module):
    """One generator G: X->Y and one discriminator D on Y, alternating G / D updates — the shared step of AEGAN and VAEGAN
    (reference Networks.py:991-1348).  As in CycleVAEGAN the discriminator runs once per step: the G phase takes its data
    gradient, the D phase its weight gradients from the same activations.  VAEGAN is written that way in the reference
    (`DGx.detach()`, `retain_graph`, :1277-1287); AEGAN re-runs D on the detached G(x) after the generator update
    (:1105-1108), which reproduces the same outputs because that update does not touch D."""
    _generators, _discriminators = ("G",), ("D",)

    def configure_optimizers(self, lr=2e-4, betas=(0.5, 0.999), clip_grad_norm=0.0, ema_decay=0.0, pool_size=0, pool_seed=0):
        return self._gan_optimizers(lr, betas, clip_grad_norm, ema_decay, pool_size, pool_seed)

    def _gan_terms(self, t, DGx, Dy):
        """The adversarial terms on one discriminator pass under the model's objective (_GanTerms) — by default LSGAN: generator
        (real -> 0, fake -> 1, Losses.py:67-83) and discriminator (real -> 1, fake -> 0, :86-102) objectives —, plus the output
        means AEGAN logs."""
        gan = _GanTerms(self.gan_objective, Dy, DGx)
        t["gan_g_real"], t["d_y_mean"] = gan.g_real()
        t["gan_g_fake"], t["d_gx_mean"] = gan.g_fake()
        t["gan_g"] = ops.weighted_sum([t["gan_g_real"], t["gan_g_fake"]], [1.0, 1.0])
        t["D_loss_real"], _ = gan.d_real()
        t["D_loss_fake"], _ = gan.d_fake()
        t["D_loss"] = ops.weighted_sum([t["D_loss_real"], t["D_loss_fake"]], [1.0, 1.0])

    def _pooled_d_terms(self, t, Gx):
        """D's fake term with an image history pool (_PoolMixin; CycleVAEGAN._pooled_d_terms).  VAEGAN's D_loss_backward stays the
        real term: its fake term is a constant of the backward with or without a pool."""
        fake = Gx.detach()
        shown, extra = self._shown_to("D", fake)
        if extra:
            t["D_loss_fake"], _ = _GanTerms(self.gan_objective, None, self.D(shown)).d_fake()
            t["D_loss"] = ops.weighted_sum([t["D_loss_real"], t["D_loss_fake"]], [1.0, 1.0])
        if self.debug_mode:
            self._debug_store().update(fake=fake, d_fake=shown)

    def training_step(self, batch):
        _refuse_training_in_ema_scope(self)
        self._check_configured()
        self.optimizer_G.zero_grad()
        t, Gx = self._losses(batch, True)
        if self.image_pools:
            self._pooled_d_terms(t, Gx)
        self._alternating_step(t["G_loss"], t.get("D_loss_backward", t["D_loss"]))
        return _report(self, t, self._fm_spec(_kl_keys(self, self._TRAIN, True)), True, **_kl_host(self, True))

    def validation_step(self, batch):
        with torch.no_grad():
            t, Gx = self._losses(batch)
            return _report(self, t, self._fm_spec(_kl_keys(self, self._VALIDATION, False)), False, Gx=Gx)


class AEGAN(_SingleGAN):
    """Autoencoder generator + discriminator: L1(G(x), y) + lambda_gan * LSGAN + lambda_identity * L1(G(y), y)
    (reference Networks.py:991-1188)."""
    _TRAIN = (_same("G_loss", "D_loss", "D_loss_real", "D_loss_fake", "loss_trans") + (("loss_gan_g", "gan_g"),)
              + _same("loss_identity", "d_y_mean", "d_gx_mean"))
    _VALIDATION = ((("total_loss", ("G_loss", "D_loss")),) + _same("G_loss", "D_loss", "D_loss_real", "D_loss_fake", "loss_trans")
                   + (("loss_gan_g", "gan_g"), ("loss_gan_g_real", "gan_g_real"), ("loss_gan_g_fake", "gan_g_fake"))
                   + _same("loss_identity") + _GX)

    def __init__(self):
        super().__init__()
        self.G = Autoencoder()
        self.D = Discriminator()
        self.apply(self._init_weights_)
        self.optimizer_G = None
        self.optimizer_D = None
        self.grad_reducer = None
        self.loss_trans_fn = None
        self.loss_gan_gen_fn = None
        self.loss_gan_disc_fn = None
        self.loss_identity_fn = None
        self.lambda_gan = 0
        self.lambda_identity = 0

    def _init_weights_(self, module):
        _kaiming_relu_init(module)

    def forward(self, x, y):
        x, y = ops.to_nhwc(x), ops.to_nhwc(y)
        Gx = self.G(x)
        Gy = self.G(y)
        return Gx, Gy, self.D(Gx), self.D(y)

    def configure_loss(self, **kwargs):
        _refuse_swd(self, kwargs)
        _refuse_kl_control(self, kwargs)
        self.loss_trans_fn = TranslationLoss()
        self.loss_gan_gen_fn, self.loss_gan_disc_fn = _configure_gan(self, kwargs)
        self.loss_identity_fn = TranslationLoss()
        self.lambda_gan = kwargs.get("lambda_gan", 1.0)
        self.lambda_identity = kwargs.get("lambda_identity", 5.0)
        self._configure_fm(kwargs)

    def _check_configured(self):
        if self.optimizer_G is None or self.optimizer_D is None:
            raise ValueError("Optimizers have not been configured yet.")
        if self.loss_trans_fn is None:
            raise ValueError("Translation loss function has not been configured yet.")
        if self.loss_gan_gen_fn is None:
            raise ValueError("GAN generator loss function has not been configured yet.")
        if self.loss_gan_disc_fn is None:
            raise ValueError("GAN discriminator loss function has not been configured yet.")
        if self.loss_identity_fn is None:
            raise ValueError("Identity loss function has not been configured yet.")

    def _losses(self, batch, training=False):
        x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
        if self.fm_term is None:
            Gx, Gy, DGx, Dy = self(x, y)
            aDGx = aDy = None
        else:                                    # `forward` with the discriminator's block activations kept
            Gx, Gy = self.G(x), self.G(y)
            (aDGx, DGx), (aDy, Dy) = self._disc(self.D, Gx), self._disc(self.D, y)
        t = {"loss_trans": self.loss_trans_fn(Gx, y), "loss_identity": self.loss_identity_fn(Gy, y)}
        self._gan_terms(t, DGx, Dy)
        terms, weights = [t["loss_trans"], t["gan_g"], t["loss_identity"]], [1.0, self.lambda_gan, self.lambda_identity]
        self._add_fm(t, terms, weights, [(aDGx, aDy)])
        t["G_loss"] = ops.weighted_sum(terms, weights)
        return t, Gx

    def validation_step(self, batch):
        self._check_configured()            # the reference's AEGAN wants its optimizers even to validate (:1145)
        return super().validation_step(batch)


class VAEGAN(_SingleGAN):
    """VAE generator + discriminator: lambda_recon * L1(G(x), y) + lambda_gan * LSGAN + lambda_identity * L1(G(y), y) +
    lambda_kl * KL(mu_x, logvar_x)  (reference Networks.py:1190-1348; eps is drawn for G(x), then for G(y))."""
    _TRAIN = (_same("G_loss", "D_loss") + (("loss_gan_disc_real", "D_loss_real"), ("loss_gan_disc_fake", "D_loss_fake"))
              + _same("loss_trans") + (("loss_gan_real", "gan_g_real"), ("loss_gan_fake", "gan_g_fake"))
              + _same("loss_identity", "loss_kl"))
    _VALIDATION = ((("total_loss", ("G_loss", "D_loss")),) + _same("G_loss", "D_loss", "loss_trans")
                   + (("loss_gan_real", "gan_g_real"), ("loss_gan_fake", "gan_g_fake")) + _same("loss_identity", "loss_kl") + _GX)

    def __init__(self, latent_dim=64):
        super().__init__()
        self.G = VariationalAutoencoder(latent_dim)
        self.D = Discriminator()
        self.latent_dim = latent_dim
        self.debug_mode = False
        self.debug_info = {}
        self.optimizer_G = None             # (left unset by the reference's __init__)
        self.optimizer_D = None
        self.grad_reducer = None

    def forward(self, x, y):
        x, y = ops.to_nhwc(x), ops.to_nhwc(y)
        Gx, mu, logvar = self.G(x)
        Gy, mu_y, logvar_y = self.G(y)
        return Gx, mu, logvar, Gy, mu_y, logvar_y, self.D(Gx), self.D(y)

    def configure_loss(self, **kwargs):
        _refuse_swd(self, kwargs)
        self.translation_loss = TranslationLoss()
        self.gan_loss_gen, self.gan_loss_disc = _configure_gan(self, kwargs)
        self.identity_loss = TranslationLoss()
        self.kl_loss = _configure_kl(self, kwargs)
        self.lambda_gan = kwargs.get("lambda_gan", 1.0)
        self.lambda_identity = kwargs.get("lambda_identity", 5.0)
        self.lambda_recon = kwargs.get("lambda_recon", 1.0)
        self._configure_fm(kwargs)

    def enable_debug_mode(self, enabled=True):
        self.debug_mode = enabled

    def _check_configured(self):
        if self.optimizer_G is None or self.optimizer_D is None:
            raise ValueError("Optimizers have not been configured yet.")

    def _losses(self, batch, training=False):
        x, y = ops.to_nhwc(batch["x"]), ops.to_nhwc(batch["y"])
        if self.fm_term is None:
            Gx, mu, logvar, Gy, _, _, DGx, Dy = self(x, y)
            aDGx = aDy = None
        else:                                    # `forward` with the discriminator's block activations kept
            (Gx, mu, logvar), (Gy, _, _) = self.G(x), self.G(y)
            (aDGx, DGx), (aDy, Dy) = self._disc(self.D, Gx), self._disc(self.D, y)
        t = {"loss_trans": self.translation_loss(Gx, y), "loss_identity": self.identity_loss(Gy, y)}
        kl, kl_objective, _ = _kl_terms(self.kl_loss, [(mu, logvar)])
        t.update(kl)
        self._gan_terms(t, DGx, Dy)
        terms = [t["loss_trans"], t["gan_g"], t["loss_identity"], kl_objective]
        weights = [self.lambda_recon, self.lambda_gan, self.lambda_identity, _kl_weight(self, training)]
        self._add_fm(t, terms, weights, [(aDGx, aDy)])
        t["G_loss"] = ops.weighted_sum(terms, weights)
        # the reference detaches the discriminator OUTPUT of the fake branch (`gan_loss_disc(Dy, DGx.detach())`, :1277),
        # not its input: the fake term is a constant in D_loss and only (1 - D(y))^2 reaches D's parameters.  Kept as
        # written — D_loss reports both terms, the backward pass sees the real one.
        t["D_loss_backward"] = t["D_loss_real"]
        return t, Gx

    def training_step(self, batch):
        m = super().training_step(batch)
        if self.debug_mode:
            m["debug_info"] = self.debug_info
        return m
