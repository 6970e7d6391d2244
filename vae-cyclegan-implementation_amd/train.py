#!/usr/bin/env python3
"""Training driver with the reference's `train.py` CLI for the hot path.

Kept from the reference (train.py:588-656): every flag name and default.  Added: `--dataset synthetic`
(on-device U[0,1) batches, the benchmark input), `--latent_dim` (the reference's README mentions it,
its argparse lacks it: create_model always used 64), `--steps_per_epoch`, `--seed`, and the BASELINE
aliases `ae` / `vae_cyclegan` for `--architecture`.  Under `torch.distributed.run` each rank trains
its shard of the global batch and gradients are exchanged by `parallel.GradReducer` (RCCL).

Built beyond the three benchmarked architectures: every architecture of the reference's factory,
`validate`, the checkpoint wire format with `--resume`, the pretraining hand-over (`--pretrained_double*`).
Out of scope, as in SURVEY.md §2: TensorBoard and the reference's PIL / torchvision dataset classes (`Data_Manager.py`).

`create_model` and `train_epoch` mirror the reference's functions of the same name (train.py:43-128).
"""
import argparse
import gc
import json
import math
import os
import sys
import time
from datetime import datetime
from pathlib import Path

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # RCCL across processes needs dmabuf IPC on this driver
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")        # kernel arguments in device memory: shorter dispatch gaps (package __init__)

import numpy as np  # noqa: E402
import torch  # noqa: E402

if __package__ in (None, ""):
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    Networks, ops, parallel, utils, input_pipeline = _pkg.Networks, _pkg.ops, _pkg.parallel, _pkg.utils, _pkg.input_pipeline
    IMAGE_TERMS = _pkg.Losses.IMAGE_TERMS
else:
    from . import Networks, input_pipeline, ops, parallel, utils
    from .Losses import IMAGE_TERMS

ALIASES = {"ae": "autoencoder", "vae_cyclegan": "cyclevaegan"}
REFERENCE_ARCHS = ["autoencoder", "doubleae", "doublevae", "vae", "aegan", "vaegan", "cycleae", "cyclevae",
                   "cycleaegan", "cyclevaegan"]
BUILT = tuple(REFERENCE_ARCHS)
SSIM_ARCHS = ("autoencoder", "vae", "cycleaegan", "cyclevaegan")     # the models whose configure_loss takes Losses.IMAGE_TERMS (named for the first)
SWD_ARCHS = ("cycleae", "cyclevae", "cycleaegan", "cyclevaegan")       # the models whose configure_loss builds the sliced Wasserstein term
KL_ARCHS = ("vae", "vaegan", "cyclevae", "cyclevaegan", "doublevae")    # the models with a KL term (Networks.KL_MODELS)
KL_DEFAULTS = {"kl_free_bits": 0.0, "kl_anneal_steps": 0, "kl_cycles": 1, "kl_ramp": 1.0}
IMAGE_TERM_HELP = {                  # --lambda_<key>, per row of Losses.IMAGE_TERMS
    "ssim": "weight of the structural term 1 - SSIM",
    "grad": "weight of the multi-scale gradient-matching term (an L1 on the finite differences of generated - target)",
    "freq": "weight of the focal frequency term (the weighted squared distance between the 2-D spectra of generated and target)",
}


def create_model(architecture, paired=True, latent_dim=64):
    """reference train.py:43-77 (which never passes latent_dim)."""
    architecture = ALIASES.get(architecture, architecture)
    if architecture == "autoencoder":
        model = Networks.Autoencoder()
        print("Created Autoencoder")
    elif architecture == "vae":
        model = Networks.VariationalAutoencoder(latent_dim=latent_dim)
        print("Created Variational Autoencoder")
    elif architecture == "doubleae":
        model = Networks.DoubleAutoencoder()
        print("Created Double Autoencoder (shared encoder + 2 decoders)")
    elif architecture == "doublevae":
        model = Networks.DoubleVariationalAutoencoder(latent_dim=latent_dim)
        print("Created Double VAE (shared encoder + 2 VAE blocks + 2 decoders)")
    elif architecture == "aegan":
        model = Networks.AEGAN()
        print("Created AE-GAN")
    elif architecture == "vaegan":
        model = Networks.VAEGAN(latent_dim=latent_dim)
        print("Created VAE-GAN")
    elif architecture == "cycleae":
        model = Networks.CycleAE(paired=paired)
        print(f"Created Cycle Autoencoder ({'paired' if paired else 'unpaired'} mode)")
    elif architecture == "cyclevae":
        model = Networks.CycleVAE(latent_dim=latent_dim, paired=paired)
        print(f"Created Cycle VAE ({'paired' if paired else 'unpaired'} mode)")
    elif architecture == "cycleaegan":
        model = Networks.CycleAEGAN(paired=paired)
        print(f"Created Cycle AE-GAN ({'paired' if paired else 'unpaired'} mode)")
    elif architecture == "cyclevaegan":
        model = Networks.CycleVAEGAN(latent_dim=latent_dim, paired=paired)
        print(f"Created Cycle VAE-GAN ({'paired' if paired else 'unpaired'} mode)")
    else:
        raise ValueError(f"Unknown architecture: {architecture}")
    return model


class SyntheticLoader:
    """len()-able iterable of {'x','y'} batches drawn on the device: x, y ~ U[0,1), (B,3,S,S)."""

    def __init__(self, batch_size, image_size, steps, device, seed=1234, rank=0, same_xy=False, epoch=0):
        self.b, self.s, self.steps, self.dev = batch_size, image_size, steps, device
        self.seed, self.rank, self.same_xy, self.epoch = seed, rank, same_xy, epoch

    def __len__(self):
        return self.steps

    def __iter__(self):
        nq = (self.b * 3 * self.s * self.s + 3) // 4
        for i in range(self.steps):
            base = (((self.epoch * self.steps + i) * 64 + self.rank) * 2) * nq
            x = ops.rand_uniform((self.b, 3, self.s, self.s), self.dev, self.seed, base)
            y = x if self.same_xy else ops.rand_uniform((self.b, 3, self.s, self.s), self.dev, self.seed, base + nq)
            yield {"x": x, "y": y}


_FROZEN = [False]


def _freeze_long_lived_objects():
    """Once per process: collect, then move the survivors (modules, parameters, ctypes tables) out of the cyclic GC's way.
    A full collection walks all of them (~30 ms of host time, with the GPU idle behind it); freezing every epoch would pin
    each epoch's garbage for good, so it is done once."""
    if not _FROZEN[0]:
        gc.collect()
        gc.freeze()
        _FROZEN[0] = True


def train_epoch(model, dataloader, device, args, writer=None, epoch=None):
    """reference train.py:80-128: per-batch training_step, metric sums averaged by len(dataloader),
    G_loss as the headline loss.  The reference also runs one extra train-mode forward per batch for a
    visualisation tensor that its caller never uses (:112-117); it is reproduced only with
    --reference_viz_forward (it advances the eps stream and costs a full forward)."""
    model.train()
    total_loss = 0.0
    loss_components = {}
    last_output = last_x = last_y = None
    _freeze_long_lived_objects()
    for batch in dataloader:
        batch["x"] = batch["x"].to(device)
        batch["y"] = batch["y"].to(device)
        metrics = model.training_step(batch)
        total_loss += metrics["G_loss"]
        for key, value in metrics.items():
            loss_components[key] = loss_components.get(key, 0.0) + value
        last_x, last_y = batch["x"], batch["y"]
        if getattr(args, "reference_viz_forward", False):
            with torch.no_grad():
                if isinstance(model, (Networks.Autoencoder, Networks.VariationalAutoencoder)):
                    last_output = model(last_x)[0]
                else:
                    last_output = model(last_x, last_y)[0]
    n = len(dataloader)
    if n > 0:
        return total_loss / n, {k: v / n for k, v in loss_components.items()}, last_output, last_x, last_y
    return float("nan"), {k: float("nan") for k in loss_components}, last_output, last_x, last_y


def validate(model, dataloader, device, args):
    """reference train.py:131-171: model.eval(), forward-only `validation_step` per batch, metrics averaged over
    len(dataloader) with G_loss as the headline; returns (avg_loss, avg_components, last Gx, last Fy, last x, last y).
    Eval mode changes one thing on this path: the discriminators' spectral norm uses the stored u, v as they are."""
    model.eval()
    total_loss = 0.0
    loss_components = {}
    last_Gx = last_Fy = last_x = last_y = None
    with torch.no_grad():
        for batch in dataloader:
            batch["x"] = batch["x"].to(device)
            batch["y"] = batch["y"].to(device)
            metrics = model.validation_step(batch)
            Gx = metrics.pop("Gx")
            Fy = metrics.pop("Fy", None)            # only the Cycle models return it
            total_loss += metrics["G_loss"]
            for key, value in metrics.items():
                loss_components[key] = loss_components.get(key, 0.0) + value
            last_Gx, last_Fy, last_x, last_y = Gx, Fy, batch["x"], batch["y"]
    n = len(dataloader)
    red = getattr(model, "grad_reducer", None)
    if red is not None:
        # data parallel: each rank validated its shard of the test set.  Shards may differ by one batch (or be empty: a test
        # split smaller than the world size), so the ranks pool their per-batch SUMS and batch counts — the same batch-weighted
        # mean the single-process loop computes — instead of averaging per-rank means
        import torch.distributed as dist
        pooled = [None] * red.world
        dist.all_gather_object(pooled, (n, total_loss, loss_components), group=red.group)
        n = sum(p[0] for p in pooled)
        total_loss = sum(p[1] for p in pooled)
        loss_components = {}
        for _, _, comp in pooled:
            for k, v in comp.items():
                loss_components[k] = loss_components.get(k, 0.0) + v
    if n == 0:
        raise ValueError("validate(): the test set is empty (no batch on any rank): lower --test_split or skip validation")
    avg_loss, avg = total_loss / n, {k: v / n for k, v in loss_components.items()}
    return avg_loss, avg, last_Gx, last_Fy, last_x, last_y


def clip_bound(text):
    """argparse type of --clip_grad_norm: a finite bound >= 0 (0: off)."""
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not math.isfinite(value) or value < 0.0:
        raise argparse.ArgumentTypeError(f"--clip_grad_norm must be finite and >= 0 (0 switches clipping off), got {text}")
    return value


def _nonneg(flag, meaning):
    """argparse type of the --lambda_<key> of Losses.IMAGE_TERMS and of --freq_alpha: a finite number >= 0."""
    def parse(text):
        try:
            value = float(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not a number: {text!r}")
        if not math.isfinite(value) or value < 0.0:
            raise argparse.ArgumentTypeError(f"{flag} must be finite and >= 0{meaning}, got {text}")
        return value
    return parse


def _at_least(flag, least, meaning):
    """argparse type of --kl_anneal_steps and --kl_cycles: an integer >= `least`."""
    def parse(text):
        try:
            value = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not an integer: {text!r}")
        if value < least:
            raise argparse.ArgumentTypeError(f"{flag} must be an integer >= {least}{meaning}, got {text}")
        return value
    return parse


def kl_ramp_value(text):
    """argparse type of --kl_ramp: a finite share of a cycle in (0, 1]."""
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not math.isfinite(value) or not 0.0 < value <= 1.0:
        raise argparse.ArgumentTypeError(f"--kl_ramp must be finite and lie in (0, 1], got {text}")
    return value


def kl_control_of(args):
    """configure_loss's KL keywords from `args` (also one built without the parser), checked as the parser checks them and
    refused for an architecture without a KL term."""
    kw = {name: getattr(args, name, default) for name, default in KL_DEFAULTS.items()}
    for name in kw:
        if isinstance(kw[name], bool) or not isinstance(kw[name], (int, float)) or not math.isfinite(kw[name]):
            raise ValueError(f"--{name} must be a finite number, got {kw[name]!r}")
    if kw["kl_free_bits"] < 0.0:
        raise ValueError(f"--kl_free_bits must be finite and >= 0 (0: no floor), got {kw['kl_free_bits']}")
    for name, least in (("kl_anneal_steps", 0), ("kl_cycles", 1)):
        if int(kw[name]) != kw[name] or kw[name] < least:
            raise ValueError(f"--{name} must be an integer >= {least}, got {kw[name]}")
    if not 0.0 < kw["kl_ramp"] <= 1.0:
        raise ValueError(f"--kl_ramp must be finite and lie in (0, 1], got {kw['kl_ramp']}")
    given = [name for name, default in KL_DEFAULTS.items() if kw[name] != default]
    if given and args.architecture not in KL_ARCHS:
        raise ValueError(f"--{given[0]} is supported by {', '.join(KL_ARCHS)} only, not by {args.architecture}: it has no KL term, "
                         "the flag would be ignored")
    return kw


def ema_decay_value(text):
    """argparse type of --ema_decay: a finite decay in [0, 1) (0: off)."""
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not math.isfinite(value) or not 0.0 <= value < 1.0:
        raise argparse.ArgumentTypeError(f"--ema_decay must be finite and lie in [0, 1) (0 switches the averaged weights off), got {text}")
    return value


POOL_ARCHS = ("aegan", "vaegan", "cycleaegan", "cyclevaegan")       # the architectures with a discriminator


def check_image_size(architecture, image_size):
    """--image_size for the architectures with a discriminator: a multiple of 16 (the body halves the image four times) and at
    least 256 (the head's 16x16 kernel on the map of image / 16; ops.head_output_shape).  The other architectures are not
    looked at here.  Raises ValueError before the first step."""
    if ALIASES.get(architecture, architecture) not in POOL_ARCHS:
        return
    try:
        ops.head_output_shape(image_size, image_size)
    except RuntimeError as e:
        raise ValueError(f"--image_size {image_size} is not usable with {architecture}: {e}") from None


def gan_label_smooth_value(text):
    """argparse type of --gan_label_smooth: a finite amount in [0, 0.5) (0: off)."""
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not math.isfinite(value) or not 0.0 <= value < 0.5:
        raise argparse.ArgumentTypeError(f"--gan_label_smooth must be finite and lie in [0, 0.5) (0: no smoothing), got {text}")
    return value


def gan_objective_of(args):
    """configure_loss's adversarial-objective keywords from `args` (also one built without the parser), checked as the parser
    checks them: refused for an architecture without a discriminator, and the smoothing refused with the hinge."""
    objective = getattr(args, "gan_objective", "lsgan")
    smooth = getattr(args, "gan_label_smooth", 0.0)
    if objective not in ops.GAN_OBJECTIVES:
        raise ValueError(f"--gan_objective must be one of {', '.join(ops.GAN_OBJECTIVES)}, got {objective!r}")
    if isinstance(smooth, bool) or not isinstance(smooth, (int, float)) or not math.isfinite(smooth) or not 0.0 <= smooth < 0.5:
        raise ValueError(f"--gan_label_smooth must be finite and lie in [0, 0.5) (0: no smoothing), got {smooth!r}")
    architecture = ALIASES.get(args.architecture, args.architecture)
    for flag, given in (("--gan_objective", objective != "lsgan"), ("--gan_label_smooth", smooth != 0.0)):
        if given and architecture not in POOL_ARCHS:
            raise ValueError(f"{flag} is supported by {', '.join(POOL_ARCHS)} only: {architecture} has no discriminator, "
                             "the flag would be ignored")
    if objective == "hinge" and smooth != 0.0:
        raise ValueError(f"--gan_label_smooth {smooth} cannot go with --gan_objective hinge: the hinge has no target to smooth "
                         "(lsgan and logistic have)")
    return {"gan_objective": objective, "gan_label_smooth": float(smooth)}


def feature_matching_of(args):
    """configure_loss's feature-matching keywords from `args` (also one built without the parser), checked as the parser checks
    them: refused for an architecture without a discriminator, and the element-wise mode refused for an unpaired cycle model."""
    weight = getattr(args, "lambda_fm", 0.0)
    mode = getattr(args, "fm_mode", "mean")
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not math.isfinite(weight) or weight < 0.0:
        raise ValueError(f"--lambda_fm must be finite and >= 0 (0: the term is not computed), got {weight!r}")
    if mode not in ops.FM_MODES:
        raise ValueError(f"--fm_mode must be one of {', '.join(ops.FM_MODES)}, got {mode!r}")
    architecture = ALIASES.get(args.architecture, args.architecture)
    for flag, given in (("--lambda_fm", weight != 0.0), ("--fm_mode", mode != "mean")):
        if given and architecture not in POOL_ARCHS:
            raise ValueError(f"{flag} is supported by {', '.join(POOL_ARCHS)} only: {architecture} has no discriminator, "
                             "the flag would be ignored")
    unpaired = not getattr(args, "paired", False) or getattr(args, "dataset", None) == "summer2winter"
    if mode == "pair" and architecture in ("cycleaegan", "cyclevaegan") and unpaired:
        raise ValueError(f"--fm_mode pair needs batches whose images correspond, which an unpaired {architecture} run does not "
                         "have (--paired, or --fm_mode mean: match the expected features)")
    return {"lambda_fm": float(weight), "fm_mode": mode}


class _Parser(argparse.ArgumentParser):
    """The checks that look at two flags at once run when the command line is parsed, before anything touches the device."""

    def parse_known_args(self, args=None, namespace=None):
        parsed, rest = super().parse_known_args(args, namespace)
        try:
            gan_objective_of(parsed)
            feature_matching_of(parsed)
        except ValueError as e:
            self.error(str(e))
        return parsed, rest


def pool_size_value(text):
    """argparse type of --pool_size: an integer >= 0 (0: off)."""
    try:
        value = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}")
    if value < 0:
        raise argparse.ArgumentTypeError(f"--pool_size must be an integer >= 0 (0 switches the image history pool off), got {text}")
    return value


def build_parser():
    p = _Parser(description="Train VAE-CycleGAN models (MI355X-native path)")
    p.add_argument("--architecture", type=str, default="autoencoder", choices=REFERENCE_ARCHS + list(ALIASES))
    p.add_argument("--paired", action="store_true", default=False)
    p.add_argument("--unpaired", dest="paired", action="store_false")
    p.add_argument("--pretrained_doubleae", type=str, default=None)
    p.add_argument("--pretrained_doublevae", type=str, default=None)
    p.add_argument("--data_dir", type=str, default="dataset")
    p.add_argument("--source_modality", type=str, default=None)
    p.add_argument("--target_modality", type=str, default=None)
    p.add_argument("--image_size", type=int, default=256)
    p.add_argument("--test_split", type=float, default=0.1)
    p.add_argument("--dataset", type=str, default="hypersim", choices=["hypersim", "summer2winter", "maps", "synthetic"])
    p.add_argument("--batch_size", type=int, default=5)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--lr", type=float, default=0.0002)
    p.add_argument("--lambda_kl", type=float, default=1e-5)
    p.add_argument("--lambda_gan", type=float, default=1.0)
    p.add_argument("--lambda_identity", type=float, default=5.0)
    p.add_argument("--lambda_cycle", type=float, default=10.0)
    p.add_argument("--lambda_recon", type=float, default=1.0)
    for row in IMAGE_TERMS:
        flag = f"--lambda_{row.key}"
        p.add_argument(flag, type=_nonneg(flag, " (0: the term is not computed)"), default=0.0,
                       help=IMAGE_TERM_HELP[row.key] + " beside the L1 (" + ", ".join(SSIM_ARCHS) + "); 0: not computed")
    p.add_argument("--grad_scales", type=int, default=4, choices=(1, 2, 3, 4),
                   help="number of scales of the gradient-matching term; scale s keeps every 2^s-th pixel")
    p.add_argument("--freq_alpha", type=_nonneg("--freq_alpha", ""), default=1.0,
                   help="exponent of the focal frequency term's spectrum weight |difference|^alpha; 0: an unweighted spectral MSE")
    p.add_argument("--lambda_msssim", type=_nonneg("--lambda_msssim", " (0: the term is not computed)"), default=0.0,
                   help="weight of the multi-scale structural term 1 - MS-SSIM (the SSIM window over a 2x2 mean pyramid: shading, "
                        "regional contrast and large shapes, which --lambda_ssim's one scale does not see) beside the L1 ("
                        + ", ".join(SSIM_ARCHS) + "); 0: not computed")
    p.add_argument("--msssim_scales", type=int, default=5, choices=(1, 2, 3, 4, 5),
                   help="levels of the multi-scale structural term's pyramid; --image_size >> (scales - 1) must be at least 11 "
                        "(5 scales: 176)")
    p.add_argument("--lambda_swd", type=_nonneg("--lambda_swd", " (0: the term is not computed)"), default=0.0,
                   help="weight of the sliced Wasserstein term swd(G(x), y) + swd(F(y), x): a distance between the patch "
                        "distributions of the translated batch and of the other domain's batch, which needs no pairing and no "
                        "discriminator (" + ", ".join(SWD_ARCHS) + "); 0: not computed")
    p.add_argument("--swd_levels", type=int, default=3, choices=(1, 2, 3),
                   help="levels of the sliced Wasserstein term's 2x2 box pyramid (a level needs sides of at least 16)")
    p.add_argument("--kl_free_bits", type=_nonneg("--kl_free_bits", " (0: no floor)"), default=0.0,
                   help="free-bits floor of the KL term, in nats per latent channel (" + ", ".join(KL_ARCHS) + "): a channel whose "
                        "mean KL is at or below it is no longer penalised, so none collapses to zero information; loss_kl stays "
                        "the plain KL, loss_kl_fb and kl_active report the floored term and the share of channels above the "
                        "floor; 0: no floor")
    p.add_argument("--kl_anneal_steps", type=_at_least("--kl_anneal_steps", 0, " (0: a constant weight)"), default=0,
                   help="anneal the KL weight: climb from 0 to --lambda_kl over this many generator steps per cycle (kl_weight "
                        "reports it; validation always uses the full weight; --resume continues the schedule); 0: constant")
    p.add_argument("--kl_cycles", type=_at_least("--kl_cycles", 1, ""), default=1,
                   help="number of annealing cycles of --kl_anneal_steps steps each (1: one warm-up; 4 with --kl_ramp 0.5: the "
                        "cyclical schedule), after which the weight stays at --lambda_kl")
    p.add_argument("--kl_ramp", type=kl_ramp_value, default=1.0,
                   help="share of each annealing cycle spent climbing; the weight is --lambda_kl for the rest of the cycle")
    p.add_argument("--clip_grad_norm", type=clip_bound, default=0.0,
                   help="clip each optimizer's gradient to this global 2-norm inside the fused Adam step (every architecture); "
                        "a step whose gradient holds a NaN / Inf is skipped; 0: off")
    p.add_argument("--ema_decay", type=ema_decay_value, default=0.0,
                   help="keep an exponential moving average of the generator weights with this decay (e.g. 0.999, warmed up from "
                        "the first step); the test loss that selects best_model.pth is then the averaged weights', and test.py / "
                        "translate.py --ema load them; 0: off")
    p.add_argument("--pool_size", type=pool_size_value, default=0,
                   help="image history pool of this many generated images per discriminator (" + ", ".join(POOL_ARCHS) + "): each "
                        "fake is shown to its discriminator as itself or, half of the time once the pool is full, exchanged "
                        "against a random stored one; 50 is the customary value; 0: off")
    p.add_argument("--gan_objective", type=str, default="lsgan", choices=ops.GAN_OBJECTIVES,
                   help="adversarial objective of the models with a discriminator (" + ", ".join(POOL_ARCHS) + "): lsgan, the "
                        "reference's least squares; hinge; logistic, the non-saturating cross-entropy — the two to reach for "
                        "where the least-squares terms saturate, as they do on the patch logits above 256 px")
    p.add_argument("--gan_label_smooth", type=gan_label_smooth_value, default=0.0,
                   help="one-sided label smoothing: the discriminator's real target becomes 1 - S (lsgan, logistic; not hinge); "
                        "0: off")
    p.add_argument("--lambda_fm", type=_nonneg("--lambda_fm", " (0: the term is not computed)"), default=0.0,
                   help="weight of the discriminator feature-matching term in the generator objective (" + ", ".join(POOL_ARCHS)
                        + "): the generator is also asked to reproduce the activations of the discriminator's four blocks on real "
                        "images, which steadies training with --gan_objective hinge, small batches and the patch head; 10 is the "
                        "customary value; the discriminator update is not touched; 0: not computed")
    p.add_argument("--fm_mode", type=str, default="mean", choices=ops.FM_MODES,
                   help="what the feature-matching term compares: mean, the per-channel expected features of the two batches "
                        "(needs no pairing); pair, the activations element by element (pix2pixHD; aegan, vaegan and paired cycle "
                        "models, whose batches correspond image by image)")
    p.add_argument("--output_dir", type=str, default="runs")
    p.add_argument("--save_freq", type=int, default=10)
    p.add_argument("--log_image_freq", type=int, default=5)
    p.add_argument("--resume", type=str, default=None)
    p.add_argument("--num_workers", type=int, default=1)
    p.add_argument("--no_cuda", action="store_true")
    # additions
    p.add_argument("--latent_dim", type=int, default=64)
    p.add_argument("--steps_per_epoch", type=int, default=20, help="synthetic dataset: batches per epoch")
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--reference_viz_forward", action="store_true")
    return p


def split_indices(n, test_split, seed):
    """(train, test) sample indices of a hypersim set of n samples: the reference's random_split (train.py:208-214) as a
    permutation drawn from the run's --seed, so that test.py evaluates on exactly what a run held out."""
    order = np.random.RandomState(seed).permutation(n)
    ntrain = int((1 - test_split) * n) if test_split > 0 else n
    return order[:ntrain], order[ntrain:]


def create_dataloaders(args, device, rank, world, epoch_seed):
    """reference train.py:174-357 (create_dataloaders_hypersim / _maps / _summer2winter) on the device-side input pipeline:
    PIL decodes, the MI355X flips, crops, resamples, jitters and converts (input_pipeline.py), from the reference's directory
    layouts (hypersim: the PNG scene tree Data_Manager.py:18-138 reads; its download / HDF5 conversion is out of scope).
    Under data parallelism every rank gets the same `epoch_seed` and takes its shard of the shared per-epoch permutation
    (train and test sets alike): one epoch is one pass over the data, and `validate` averages the metrics over ranks."""
    if args.dataset == "hypersim":
        # reference train.py:174-239: one HypersimDataset with the TRAINING transforms, random_split into train / test
        mods = [m for m in (args.source_modality, args.target_modality) if m]
        if len(mods) == 2 and mods[0] == mods[1]:
            mods = mods[:1]          # the reference keys its images by modality name: two equal names are ONE image, x is y
        if not mods:
            raise ValueError("--dataset hypersim needs --source_modality (and --target_modality)")
        full = input_pipeline.HypersimFolders(os.path.join(args.data_dir, "hypersim"), mods, paired=args.paired or len(mods) == 1)
        kw = dict(num_workers=max(1, args.num_workers), same_xy=len(mods) == 1, rank=rank, world=world)
        train_idx, test_idx = split_indices(len(full), args.test_split, args.seed)
        ntrain = len(train_idx)
        print(f"Training samples: {ntrain}" + (f", Testing samples: {len(full) - ntrain}" if args.test_split > 0 else ""))
        train = input_pipeline.DeviceInputPipeline(full.subset(train_idx), args.batch_size, args.image_size, device,
                                                   recipe="hypersim", shuffle=True, seed=epoch_seed, **kw)
        test = None
        if len(test_idx):
            test = input_pipeline.DeviceInputPipeline(full.subset(test_idx), args.batch_size, args.image_size, device,
                                                      recipe="hypersim", shuffle=False, seed=epoch_seed, **kw)
        return train, test
    root = os.path.join(args.data_dir, args.dataset)
    same_xy = args.architecture in ("autoencoder", "vae")
    test_split = "test" if args.dataset == "summer2winter" else "val"
    train_src = input_pipeline.FolderPairs(root, args.dataset, "train")
    test_src = input_pipeline.FolderPairs(root, args.dataset, test_split)
    print(f"Training samples: {len(train_src)}\nTesting samples: {len(test_src)}")
    kw = dict(num_workers=max(1, args.num_workers), same_xy=same_xy, rank=rank, world=world)
    train = input_pipeline.DeviceInputPipeline(train_src, args.batch_size, args.image_size, device, recipe=args.dataset, shuffle=True,
                                               seed=epoch_seed, **kw)
    test = input_pipeline.DeviceInputPipeline(test_src, args.batch_size, args.image_size, device, recipe="test", shuffle=False,
                                              seed=epoch_seed, **kw)
    return train, test


DATASET_MODALITY_DEFAULTS = {                        # reference train.py:367-377
    "hypersim": ("depth", "normal"),
    "summer2winter": ("summer", "winter"),
    "maps": ("satellite", "map"),
    "synthetic": ("synthetic", "synthetic"),
}


def main(args):
    args.architecture = ALIASES.get(args.architecture, args.architecture)
    image_kw = {}                                    # configure_loss's keywords for the optional image terms
    for row in IMAGE_TERMS:
        name = f"lambda_{row.key}"
        weight = image_kw[name] = getattr(args, name, 0.0)        # (an args object built without the parser)
        if not math.isfinite(weight) or weight < 0.0:
            raise ValueError(f"--{name} must be finite and >= 0 (0: the term is not computed), got {weight}")
        if weight != 0.0 and args.architecture not in SSIM_ARCHS:
            raise ValueError(f"--{name} is supported by {', '.join(SSIM_ARCHS)} only, not by {args.architecture}: "
                             "the flag would be ignored")
        if row.option is not None:
            image_kw[row.option] = getattr(args, row.option, row.default)
    if image_kw["grad_scales"] not in (1, 2, 3, 4):
        raise ValueError(f"--grad_scales must be 1, 2, 3 or 4, got {image_kw['grad_scales']}")
    if not math.isfinite(image_kw["freq_alpha"]) or image_kw["freq_alpha"] < 0.0:
        raise ValueError(f"--freq_alpha must be finite and >= 0, got {image_kw['freq_alpha']}")
    lambda_msssim = image_kw["lambda_msssim"] = getattr(args, "lambda_msssim", 0.0)
    if not math.isfinite(lambda_msssim) or lambda_msssim < 0.0:
        raise ValueError(f"--lambda_msssim must be finite and >= 0 (0: the term is not computed), got {lambda_msssim}")
    if lambda_msssim != 0.0 and args.architecture not in SSIM_ARCHS:
        raise ValueError(f"--lambda_msssim is supported by {', '.join(SSIM_ARCHS)} only, not by {args.architecture}: "
                         "the flag would be ignored")
    msssim_scales = image_kw["msssim_scales"] = getattr(args, "msssim_scales", 5)
    if isinstance(msssim_scales, bool) or msssim_scales not in (1, 2, 3, 4, 5):
        raise ValueError(f"--msssim_scales must be 1, 2, 3, 4 or 5, got {msssim_scales}")
    image_size = getattr(args, "image_size", 256)
    check_image_size(args.architecture, image_size)
    if lambda_msssim != 0.0 and ops.msssim_max_scales(image_size, image_size) < msssim_scales:
        usable = ops.msssim_max_scales(image_size, image_size)
        raise ValueError(f"--image_size {image_size} is too small for --msssim_scales {msssim_scales}: the coarsest level, "
                         f"image_size >> (scales - 1), must hold the 11x11 window; "
                         + (f"the largest usable --msssim_scales is {usable}" if usable else "no --msssim_scales is usable below 11"))
    lambda_swd = image_kw["lambda_swd"] = getattr(args, "lambda_swd", 0.0)
    if not math.isfinite(lambda_swd) or lambda_swd < 0.0:
        raise ValueError(f"--lambda_swd must be finite and >= 0 (0: the term is not computed), got {lambda_swd}")
    if lambda_swd != 0.0 and args.architecture not in SWD_ARCHS:
        raise ValueError(f"--lambda_swd is supported by {', '.join(SWD_ARCHS)} only, not by {args.architecture}: "
                         "the flag would be ignored")
    image_kw["swd_levels"] = getattr(args, "swd_levels", 3)
    if image_kw["swd_levels"] not in (1, 2, 3):
        raise ValueError(f"--swd_levels must be 1, 2 or 3, got {image_kw['swd_levels']}")
    kl_kw = kl_control_of(args)
    gan_kw = gan_objective_of(args)
    fm_kw = feature_matching_of(args)
    clip = getattr(args, "clip_grad_norm", 0.0)
    if not math.isfinite(clip) or clip < 0.0:
        raise ValueError(f"--clip_grad_norm must be finite and >= 0 (0 switches clipping off), got {clip}")
    ema_decay = getattr(args, "ema_decay", 0.0)
    if not math.isfinite(ema_decay) or not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"--ema_decay must be finite and lie in [0, 1) (0 switches the averaged weights off), got {ema_decay}")
    pool_size = getattr(args, "pool_size", 0)
    if isinstance(pool_size, bool) or not isinstance(pool_size, int) or pool_size < 0:
        raise ValueError(f"--pool_size must be an integer >= 0 (0 switches the image history pool off), got {pool_size}")
    if pool_size > 0 and args.architecture not in POOL_ARCHS:
        raise ValueError(f"--pool_size is supported by {', '.join(POOL_ARCHS)} only: {args.architecture} has no discriminator, "
                         "the flag would be ignored")
    # reference train.py:362-377, in its order: the autoencoder / VAE check sees the modalities as given, THEN the
    # per-dataset defaults fill in what was not given (they name the run directory and select hypersim's frames)
    if args.architecture in ("autoencoder", "vae"):
        if args.source_modality != args.target_modality:
            raise ValueError("Source and target modalities should be the same for Autoencoder/VAE architectures.")
    default_source, default_target = DATASET_MODALITY_DEFAULTS[args.dataset]
    if args.source_modality is None:
        args.source_modality = default_source
    if args.target_modality is None:
        args.target_modality = default_target
    if args.dataset in ("summer2winter",):
        args.paired = False                          # reference train.py:380-382: unpaired data forces the unpaired objectives
    if args.no_cuda or not torch.cuda.is_available():
        raise RuntimeError("this path has no CPU implementation: an MI355X is required (the reference's own "
                           "train.py is the CPU path)")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device, pg_options=parallel.nccl_options())

    # reference train.py:395-411: a resumed run continues in its checkpoint's directory, a new one gets
    # <architecture>_<timestamp>_<source>_to_<target>_<dataset> and writes its args.json there
    if args.resume:
        if not Path(args.resume).exists():
            raise FileNotFoundError(f"No checkpoint found at {args.resume}")
        output_dir = Path(args.resume).parent
        if rank == 0:
            print(f"Using device: {device}  world size {world}\nResuming run in directory: {output_dir}")
    else:
        output_dir = Path(args.output_dir) / (f"{args.architecture}_{datetime.now().strftime('%m%d_%H%M')}_{args.source_modality}_to_"
                                              f"{args.target_modality}_{args.dataset}")
        if rank == 0:
            output_dir.mkdir(parents=True, exist_ok=True)
            with open(output_dir / "args.json", "w") as f:
                json.dump(vars(args), f, indent=2)
            print(f"Using device: {device}  world size {world}\nOutput directory: {output_dir}")

    torch.manual_seed(args.seed)                     # identical replicas
    ops.manual_seed(ops.rank_seed(args.seed, rank))  # per-rank eps stream
    model = create_model(args.architecture, paired=args.paired, latent_dim=args.latent_dim).to(device)
    if pool_size > 0:                                # the pools draw their plans per rank, as the eps streams do
        model.configure_optimizers(lr=args.lr, clip_grad_norm=clip, ema_decay=ema_decay, pool_size=pool_size,
                                   pool_seed=ops.rank_seed(args.seed, rank))
        if rank == 0:
            print(f"Image history pool: {pool_size} images per discriminator")
    else:
        model.configure_optimizers(lr=args.lr, clip_grad_norm=clip, ema_decay=ema_decay)
    if rank == 0 and (gan_kw["gan_objective"], gan_kw["gan_label_smooth"]) != ("lsgan", 0.0):
        print(f"Adversarial objective: {gan_kw['gan_objective']}, label smoothing {gan_kw['gan_label_smooth']}")
    if rank == 0 and fm_kw["lambda_fm"] > 0.0:
        print(f"Discriminator feature matching: weight {fm_kw['lambda_fm']}, mode {fm_kw['fm_mode']}")
    if ema_decay > 0.0 and rank == 0:
        print(f"Averaged generator weights (decay {ema_decay}): the test loss, and with it best_model.pth, is the averaged weights'")
    model.configure_loss(lambda_kl=args.lambda_kl, lambda_gan=args.lambda_gan, lambda_identity=args.lambda_identity,
                         lambda_cycle=args.lambda_cycle, lambda_recon=args.lambda_recon,
                         swd_seed=ops.rank_seed(args.seed, rank) % 2 ** 32, **image_kw, **kl_kw, **gan_kw, **fm_kw)      # plans per rank, as the eps streams
    if world > 1:
        parallel.attach(model)
    same_xy = args.architecture in ("autoencoder", "vae")
    # reference train.py:448-463: a pretraining checkpoint initialises the generators of a Cycle model
    if args.pretrained_doubleae is not None and args.pretrained_doublevae is not None:
        raise ValueError("Cannot specify both --pretrained_doubleae and --pretrained_doublevae")
    if args.pretrained_doubleae is not None:
        if args.architecture not in ("cycleae", "cyclevae", "cycleaegan", "cyclevaegan"):
            raise ValueError(f"--pretrained_doubleae can only be used with Cycle architectures, not {args.architecture}")
        utils.load_pretrained_doubleae_to_cycleae(model, args.pretrained_doubleae, device)
    if args.pretrained_doublevae is not None:
        if args.architecture not in ("cyclevae", "cyclevaegan"):
            raise ValueError("--pretrained_doublevae can only be used with CycleVAE or CycleVAEGAN architectures, "
                             f"not {args.architecture}")
        utils.load_pretrained_doublevae_to_cyclevae(model, args.pretrained_doublevae, device)
    start_epoch = 0
    if args.resume:                                  # reference train.py:471-477
        if rank == 0:
            print(f"Resuming from checkpoint: {args.resume}")
        start_epoch, _ = utils.load_checkpoint(model, Path(args.resume), device)
        start_epoch += 1
    if world > 1:
        # identical replicas: AFTER every load above, so that replica identity never depends on each rank having read
        # the same file; the broadcast also invalidates the weight packs of anything a load or a warm-up forward packed
        parallel.broadcast_parameters(model)
    best_test_loss = utils.LAST_EXTRAS.get("best_test_loss", float("inf")) if args.resume else float("inf")
    image_loaders = create_dataloaders(args, device, rank, world, args.seed) if args.dataset != "synthetic" else None
    for epoch in range(start_epoch, args.epochs):
        loader = image_loaders[0] if image_loaders else SyntheticLoader(args.batch_size, args.image_size, args.steps_per_epoch, device,
                                                                       args.seed, rank, same_xy, epoch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train_loss, comps, *_ = train_epoch(model, loader, device, args, epoch=epoch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rank == 0:
            ips = args.batch_size * world * len(loader) / dt
            print(f"\nEpoch {epoch + 1}/{args.epochs}\nTrain Loss: {train_loss:.4f}   ({ips:.1f} images/s)")
            for k, v in comps.items():
                print(f"  {k}: {v:.6f}")
            for k, v in comps.items():               # what the reference's unused `nan_count` was for (train.py:90)
                if k.startswith("grad_skipped"):
                    print(f"  steps skipped for a NaN / Inf gradient ({k}): {round(v * len(loader))} of {len(loader)}")
        # on the test set (reference train.py:533-537: every log_image_freq epochs); here a held-out synthetic stream.
        # validation_step has no exchange in it: every rank validates its shard of the test set and `validate` averages
        # the metrics over ranks
        if args.log_image_freq > 0 and epoch % args.log_image_freq == 0 and not (image_loaders and image_loaders[1] is None):
            test_loader = image_loaders[1] if image_loaders else SyntheticLoader(
                args.batch_size, args.image_size, max(1, args.steps_per_epoch // 10), device, args.seed + 1, rank, same_xy, epoch)
            with model.ema_scope():                  # the averaged weights, when the run keeps them; the raw ones otherwise
                test_loss, test_comps, *_ = validate(model, test_loader, device, args)
            if rank == 0:
                print(f"Test Loss: {test_loss:.4f}")
                for k, v in test_comps.items():
                    print(f"  {k}: {v:.6f}")
                if test_loss < best_test_loss:       # reference train.py:565-570
                    best_test_loss = test_loss
                    utils.save_checkpoint(model, epoch, test_loss, args, output_dir / "best_model.pth", best_test_loss,
                                          pool_images=False)
                    print(f"New best model saved (test_loss: {test_loss:.4f})")
        if rank == 0 and (epoch + 1) % args.save_freq == 0:      # reference train.py:573-575 (replicas are identical)
            utils.save_checkpoint(model, epoch, train_loss, args, output_dir / f"checkpoint_epoch_{epoch + 1}.pth", best_test_loss)
    if world > 1:
        dist.destroy_process_group()
    if rank == 0:
        print(f"\nTraining completed. Run directory: {output_dir}")


if __name__ == "__main__":
    main(build_parser().parse_args())
