#!/usr/bin/env python3
"""Apply a trained generator to whole images of any size: `python translate.py --checkpoint RUN_OR_PTH --input FILE_OR_DIR
--output DIR`.  New: the reference has no inference entry point (its test.py only walks runs/ and squeezes every sample to
--image_size squared).

The generators are fully convolutional, so a frame goes through in one piece: decoded with Pillow on host threads into a pinned
buffer, copied to the device as uint8, converted and reflect-padded to multiples of 16 there (csrc/image_io.hip), run through
the generator alone in eval mode, cropped and converted to uint8 on the device; only those bytes come back.  Frames of equal
size are batched.  No tiling: InstanceNorm statistics are taken over the whole image, so tiles would not reproduce the
whole-frame result; a batch above `ops.MAX_TRANSLATE_PIXELS` padded pixels is refused instead ("The translator").

Directions: `a2b` is G (the one generator of autoencoder / vae / aegan / vaegan), `b2a` is F of the cycle models.  For doubleae /
doublevae the two directions are the models' `translate_A_to_B` (decoder_B) and `translate_B_to_A` (decoder_A) — NOT what
test.py shows for them, which is the reconstruction decoder_A(encoder(x)) their forward returns first.

`--samples K` (variational generators): K draws per frame from ONE encoder pass — the latent's mu and logvar do not depend on eps —
decoded in chunks of as many samples as the pixel bound admits, with the running mean and the per-pixel spread of the draws
accumulated on the device (csrc/sample_stats.hip; DESIGN.md, "Sampling translator").

`--interpolate N` (variational generators): N frames between each two consecutive inputs, decoded from a path through latent
space between the two frames' latent means — every frame encoded once, the path (spherical by default) computed on the device
(csrc/latent_path.hip; DESIGN.md, "Interpolating translator").
"""
import argparse
import json
import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

if __package__ in (None, ""):
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    ops, utils, input_pipeline = _pkg.ops, _pkg.utils, _pkg.input_pipeline
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")
else:
    from . import input_pipeline, ops, train, utils

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")
METRIC_NAMES = ("l1", "mse", "psnr", "ssim")
ONE_GENERATOR = ("autoencoder", "vae", "aegan", "vaegan")
VARIATIONAL = ("vae", "vaegan", "cyclevae", "cyclevaegan", "doublevae")


# ------------------------------------------------------------------ the model
def load_generator(checkpoint_or_run_dir, architecture=None, latent_dim=None, paired=None, device="cuda", ema=False):
    """(model in eval mode, architecture) from a run directory (its args.json + best_model.pth, as test.load_model) or from a
    bare .pth plus the arguments args.json would have given.  Parameters only: no optimizer state is loaded.  `ema`: the
    checkpoint's averaged generator weights instead of the raw ones (a KeyError if it has none)."""
    path = Path(checkpoint_or_run_dir)
    if path.is_dir():
        with open(path / "args.json") as f:
            a = json.load(f)
        architecture = architecture or a["architecture"]
        latent_dim = a.get("latent_dim", 64) if latent_dim is None else latent_dim
        paired = a.get("paired", True) if paired is None else paired
        path = path / "best_model.pth"
    if architecture is None:
        raise ValueError("a bare checkpoint file needs --architecture (a run directory has it in args.json)")
    architecture = train.ALIASES.get(architecture, architecture)
    model = train.create_model(architecture, paired=True if paired is None else paired,
                               latent_dim=64 if latent_dim is None else latent_dim).to(device)
    utils.load_model_weights(model, str(path), ema=ema)
    model.eval()
    return model, architecture


def generator_of(model, architecture, direction="a2b"):
    """The function logical nhwc batch -> translated batch of one direction of a model (see the module docstring)."""
    arch = train.ALIASES.get(architecture, architecture)
    if direction not in ("a2b", "b2a"):
        raise ValueError(f"direction must be 'a2b' or 'b2a', got {direction!r}")
    if arch not in train.REFERENCE_ARCHS:
        raise ValueError(f"Unknown architecture: {architecture}")
    if direction == "b2a" and arch in ONE_GENERATOR:
        raise ValueError(f"{arch} has one generator (A -> B): there is no b2a direction to run")
    if arch == "autoencoder":
        return model
    if arch == "vae":
        return lambda x: model(x)[0]
    if arch in ("doubleae", "doublevae"):
        return model.translate_A_to_B if direction == "a2b" else model.translate_B_to_A
    gen = model.G if direction == "a2b" else model.F
    return (lambda x: gen(x)[0]) if arch in VARIATIONAL else gen


def _latent_dim(model):
    for m in model.modules():
        if hasattr(m, "latent_dim") and hasattr(m, "muConv"):
            return m.latent_dim
    raise RuntimeError("eps='mean' on a variational architecture whose model has no variational block")


def run_generator(model, architecture, x, direction="a2b", eps="sample", seed=1234):
    """One direction of `model` on a logical (N, 3, Hp, Wp) batch (Hp, Wp multiples of 16), in eval mode without autograd.
    eps: "sample" draws the reparameterisation noise from the ops stream (seeded with `seed` first unless it is None: the stream
    goes on where it is); "mean" injects zeros, so a variational generator decodes mu and the output is deterministic."""
    if eps not in ("sample", "mean"):
        raise ValueError(f"eps must be 'sample' or 'mean', got {eps!r}")
    arch = train.ALIASES.get(architecture, architecture)
    gen = generator_of(model, arch, direction)
    n, _, hp, wp = x.shape
    if hp % 16 or wp % 16:
        raise RuntimeError(f"run_generator: {hp}x{wp} is not a multiple of 16 on both sides (ops.image_load pads)")
    ops.check_translate_size(n, hp, wp)
    model.eval()
    try:
        if arch in VARIATIONAL:
            if eps == "mean":
                ops.inject_eps([torch.zeros((n, _latent_dim(model), hp // 16, wp // 16), dtype=torch.float32, device=x.device)])
            elif seed is not None:
                ops.manual_seed(seed)
        with torch.no_grad():
            return gen(ops.to_nhwc(x))
    finally:
        ops.inject_eps([])


def _as_frames(frames):
    """uint8 (N, H, W, C) tensor (wherever it lives) of an array, a tensor or a list of same-sized ones; grey (H, W) gets C = 1."""
    if isinstance(frames, (list, tuple)):
        items = [torch.from_numpy(np.array(f)) if not isinstance(f, torch.Tensor) else f for f in frames]      # a copy: Pillow's arrays are read-only
        items = [f.unsqueeze(-1) if f.dim() == 2 else f for f in items]
        if len({tuple(f.shape) for f in items}) != 1:
            raise ValueError(f"frames of one call must have one size, got {sorted({tuple(f.shape) for f in items})}")
        frames = torch.stack(items)
    elif not isinstance(frames, torch.Tensor):
        frames = torch.as_tensor(np.asarray(frames))
    if frames.dim() == 3:
        frames = frames.unsqueeze(0) if frames.shape[-1] in (1, 3, 4) else frames.unsqueeze(-1)
    if frames.dim() != 4 or frames.dtype != torch.uint8 or frames.shape[3] not in (1, 3, 4):
        raise ValueError(f"expected uint8 frames (N, H, W, C) with C in (1, 3, 4), got {frames.dtype} {tuple(frames.shape)}")
    return frames


def translate_padded(model, architecture, frames, direction="a2b", eps="sample", seed=1234, device=None):
    """(generator output as a logical (N, 3, Hp, Wp) batch, window (top, left, H, W) of the frames inside it)."""
    frames = _as_frames(frames)
    n, h, w, _ = frames.shape
    generator_of(model, architecture, direction)                    # a wrong direction fails before anything is copied
    ops.check_translate_size(n, h, w)                               # ... and so does a frame that cannot go through
    device = device or next(model.parameters()).device
    x, window = ops.image_load(frames.to(device, non_blocking=True))
    return run_generator(model, architecture, x, direction, eps, seed), window


def translate_images(model, architecture, frames, direction="a2b", eps="sample", seed=1234, return_float=False, device=None):
    """uint8 frames (N, H, W, C) (array, tensor or list of same-sized ones; C = 1, 3 or 4) -> the translated frames on the device,
    uint8 (N, H, W, 3) (`return_float`: fp32 clamped to [0, 1]).  Pads by reflection to multiples of 16, runs the generator of
    `direction` alone, crops."""
    y, window = translate_padded(model, architecture, frames, direction, eps, seed, device)
    return ops.to_display_hw(y, window, uint8=not return_float)


# ------------------------------------------------------------------ K draws per frame
def sampler_of(model, architecture, direction="a2b"):
    """(latent, decode) of one direction of a variational model: x -> (mu, logvar) and z -> translated batch, the two halves of
    what `generator_of` returns.  Refuses what has no latent distribution to draw from."""
    arch = train.ALIASES.get(architecture, architecture)
    if arch in train.REFERENCE_ARCHS and arch not in VARIATIONAL:
        raise ValueError(f"{arch} is not variational ({', '.join(VARIATIONAL)} are): its output is one image, there is nothing to sample")
    generator_of(model, arch, direction)                            # unknown architecture, wrong direction
    if arch == "vae":
        return model.latent, model.decode
    if arch == "doublevae":
        side = "B" if direction == "a2b" else "A"
        return (lambda x: model.latent(x, side)), (lambda z: model.decode(z, side))
    gen = model.G if direction == "a2b" else model.F
    return gen.latent, gen.decode


def sample_chunks(n, hp, wp, samples, chunk=None):
    """[(first, k)]: the samples 0 .. samples - 1 of n frames of hp x wp padded pixels in decoder batches of n * k images, k the
    largest with n * k * hp * wp <= ops.MAX_TRANSLATE_PIXELS (`chunk`: at most this many)."""
    if samples < 1 or n < 1 or n * hp * wp > ops.MAX_TRANSLATE_PIXELS:
        raise ValueError(f"sample_chunks: {samples} sample(s) of {n} frame(s) of {hp}x{wp}")
    if chunk is not None and chunk < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    k = ops.MAX_TRANSLATE_PIXELS // (n * hp * wp)
    k = min(k, samples) if chunk is None else min(k, samples, chunk)
    return [(first, min(k, samples - first)) for first in range(0, samples, k)]


def _check_sampling(samples, temperature):
    if samples < 2:
        raise ValueError(f"samples must be at least 2 (a spread needs two draws), got {samples}; one draw is translate_images")
    if not (math.isfinite(temperature) and temperature >= 0):
        raise ValueError(f"temperature must be finite and >= 0, got {temperature}")


def sample_padded(model, architecture, x, window, samples, direction="a2b", temperature=1.0, eps=None, chunk=None, spread_gain=2.0,
                  target=None, debug=False):
    """`sample_images` on a loaded logical (N, 3, Hp, Wp) batch whose frames are `window` of it; the eps stream goes on where it
    is.  `target` (a batch like x): adds "metrics" (N, 4) of the mean image and "sample_metrics" (N, K, 4), on the device."""
    latent, decode = sampler_of(model, architecture, direction)
    _check_sampling(samples, temperature)
    n, _, hp, wp = x.shape
    top, left, h, w = window
    plan = sample_chunks(n, hp, wp, samples, chunk)
    model.eval()
    out = {}
    with torch.no_grad():
        mu, logvar = latent(x)                                      # the one encoder pass
        if eps is None:
            offset = ops.reserve_eps_many(mu, samples)              # the stream advances once per batch, not per chunk
        elif tuple(eps.shape) != (n, samples) + tuple(mu.shape[1:]):
            raise RuntimeError(f"eps has shape {tuple(eps.shape)}, expected {(n, samples) + tuple(mu.shape[1:])}")
        else:
            eps, offset = eps.to(x.device), None
        drawn = torch.empty((n, samples, h, w, 3), dtype=torch.float32 if debug else torch.uint8, device=x.device)
        mean = ops.logical_of(torch.empty((n, hp, wp, 4), dtype=torch.float32, device=x.device), 3)
        m2 = ops.logical_of(torch.empty((n, hp, wp, 4), dtype=torch.float32, device=x.device), 3)
        used, sample_metrics = [], []
        for first, k in plan:
            z, e = ops.reparameterize_many(mu, logvar, samples, first, k, eps=None if eps is None else eps[:, first:first + k],
                                           temperature=temperature, seed_offset=offset)
            y = decode(z)                                           # (N * k, 3, Hp, Wp), sample j of frame n at n * k + j
            drawn[:, first:first + k] = ops.to_display_hw(y, window, uint8=not debug).view(n, k, h, w, 3)
            ops.sample_accumulate(y, mean, m2, k, first)
            if target is not None:
                t = ops.logical_of(ops.as_phys(target).repeat_interleave(k, dim=0), 3)
                sample_metrics.append(ops.image_metrics_hw(y, t, window).view(n, k, 4))
            if debug:
                used.append(e.reshape(n, k, *e.shape[1:]))
        (spread, spread_u8), mean_spread = ops.spread_display_hw(m2, samples, window, gain=spread_gain, uint8="both")
        out.update(samples=drawn, mean=ops.to_display_hw(mean, window, uint8=not debug), spread=spread, spread_u8=spread_u8,
                   mean_spread=mean_spread)
        if target is not None:
            out.update(metrics=ops.image_metrics_hw(mean, target, window), sample_metrics=torch.cat(sample_metrics, dim=1))
        if debug:
            out["eps"] = torch.cat(used, dim=1)
    return out


def sample_images(model, architecture, frames, samples, direction="a2b", seed=1234, temperature=1.0, eps=None, chunk=None, device=None,
                  spread_gain=2.0, debug=False):
    """`samples` >= 2 translations of each uint8 frame (as translate_images takes them) by a variational generator, from one
    encoder pass -> a dict of device tensors:
      samples      uint8 (N, K, H, W, 3), sample j of frame n drawn with z = mu + temperature * eps[n, j] * sigma;
      mean         uint8 (N, H, W, 3), the display conversion of the running mean of the clamped samples;
      spread       fp32 (N, H, W), per pixel the RMS over the channels of the unbiased sample standard deviation;
      spread_u8    uint8 (N, H, W), floor(255 min(1, spread_gain * spread) + 0.5);
      mean_spread  fp32 (N,), the mean of `spread` per frame.
    The decoder runs on chunks of samples (`sample_chunks`; `chunk` lowers the chunk size); a draw depends on (seed, n, j) only,
    not on the chunking.  seed None: the eps stream goes on where it is.  eps: (N, K, latent, Hp / 16, Wp / 16) noise instead of
    drawn one (parity runs).  debug: samples and mean as fp32 clamped to [0, 1], and "eps", the noise that was used."""
    frames = _as_frames(frames)
    n, h, w, _ = frames.shape
    sampler_of(model, architecture, direction)                      # refusals come before anything is copied
    _check_sampling(samples, temperature)
    ops.check_translate_size(n, h, w)
    device = device or next(model.parameters()).device
    x, window = ops.image_load(frames.to(device, non_blocking=True))
    if eps is None and seed is not None:
        ops.manual_seed(seed)
    return sample_padded(model, architecture, x, window, samples, direction, temperature, eps, chunk, spread_gain, debug=debug)


# ------------------------------------------------------------------ N frames between two inputs
def _check_interpolation(steps, mode):
    if steps < 1:
        raise ValueError(f"interpolate: at least 1 intermediate frame, got {steps}")
    if mode not in ops.LATENT_PATH_MODES:
        raise ValueError(f"interp_mode must be one of {', '.join(ops.LATENT_PATH_MODES)}, got {mode!r}")


def interpolate_padded(model, architecture, x, window, steps, direction="a2b", mode="slerp", chunk=None, debug=False, carry=None):
    """`interpolate_images` on a loaded logical (N, 3, Hp, Wp) batch whose frames are `window` of it.  `carry`: the latent mean
    of the frame BEFORE x[0] (a previous call's "last_mu"), which then opens the first pair: N pairs instead of N - 1, and no
    frame is encoded twice.  The result also holds "last_mu", the (1, C, h, w) latent mean of x[-1].  One frame without a carry
    gives no pair: empty tensors and its "last_mu" (how a folder starts at --batch_size 1)."""
    latent, decode = sampler_of(model, architecture, direction)
    _check_interpolation(steps, mode)
    n, _, hp, wp = x.shape
    top, left, h, w = window
    pairs = n - 1 if carry is None else n
    total = steps + 2
    plan = sample_chunks(pairs, hp, wp, total, chunk) if pairs >= 1 else []
    model.eval()
    with torch.no_grad():
        mu, _ = latent(x)                                           # the one encoder pass; the path runs on the means: no eps draw
        c = mu.shape[1]
        if carry is not None:
            if tuple(carry.shape) != (1,) + tuple(mu.shape[1:]):
                raise RuntimeError(f"carry has shape {tuple(carry.shape)}, expected {(1,) + tuple(mu.shape[1:])}")
            mu = ops.logical_of(torch.cat([ops.as_phys(carry), ops.as_phys(mu)]), c)
        out = {"last_mu": ops.logical_of(ops.as_phys(mu[-1:]).clone(), c)}
        frames = torch.empty((pairs, total, h, w, 3), dtype=torch.float32 if debug else torch.uint8, device=x.device)
        step = torch.empty((pairs, total - 1), dtype=torch.float32, device=x.device)
        stats = torch.empty((pairs, 3), dtype=torch.float64, device=x.device)
        coefs, latents, prev = [], [], None
        if pairs >= 1:
            a, b = mu[:-1], mu[1:]                                  # consecutive frames: two views of the one batch
            stats = ops.latent_pair_stats(a, b)
        for first, k in plan:
            z = ops.latent_path(a, b, steps, mode, first, k, stats=stats, return_coef=debug)
            if debug:
                z, coef = z
                coefs.append(coef)
                latents.append(z.reshape(pairs, k, *z.shape[1:]))
            y = decode(z)                                           # (P * k, 3, Hp, Wp), fraction j of pair p at p * k + (j - first)
            shown = ops.to_display_hw(y, window).view(pairs, k, h, w, 3)
            frames[:, first:first + k] = shown if debug else ops.to_display_hw(y, window, uint8=True).view(pairs, k, h, w, 3)
            # the steps between consecutive frames as the viewer sees them: the clamped frames back at pitch 4, the previous
            # chunk's last frame in front, and ONE metrics launch over the run shifted by one frame (the step from a pair's last
            # frame to the next pair's first is computed with the rest and dropped)
            lead = 0 if prev is None else 1
            run = torch.zeros((pairs, lead + k, h, w, 4), dtype=torch.float32, device=x.device)
            run[:, lead:, :, :, :3] = shown
            if lead:
                run[:, 0] = prev
            prev = run[:, -1].clone()
            if lead + k >= 2:
                flat = ops.logical_of(run.view(pairs * (lead + k), h, w, 4), 3)
                l1 = ops.image_metrics_hw(flat[1:], flat[:-1])[:, 0]
                step[:, first - lead:first + k - 1] = torch.cat([l1, l1.new_zeros(1)]).view(pairs, lead + k)[:, :lead + k - 1]
        cos = (stats[:, 2] / (stats[:, 0] * stats[:, 1]).sqrt()).clamp(-1.0, 1.0)
        out.update(frames=frames, step_l1=step, omega=torch.acos(cos).float(), norm_a=stats[:, 0].sqrt().float(),
                   norm_b=stats[:, 1].sqrt().float())
        if debug and plan:
            out.update(coef=torch.cat(coefs, dim=1), latents=torch.cat(latents, dim=1))
    return out


def interpolate_images(model, architecture, frames, steps, direction="a2b", mode="slerp", chunk=None, device=None, debug=False):
    """`steps` >= 1 frames between each two consecutive uint8 frames (as translate_images takes them; at least two) by a
    variational generator: every frame is encoded once, pair p is (frame p, frame p + 1), and the T = steps + 2 latents
    z(t_j), t_j = j / (T - 1), of each pair's path between the two latent MEANS are decoded -> a dict of device tensors:
      frames   uint8 (P, T, H, W, 3); frames[p, 0] is the translation of frame p at its latent mean, frames[p, T - 1] that of
               frame p + 1;
      omega    fp32 (P,), the angle between the two latent means (NaN where one is all zeros); norm_a, norm_b their 2-norms;
      step_l1  fp32 (P, T - 1), the mean absolute difference between consecutive decoded frames as displayed.
    mode "slerp" walks the great circle (ops.latent_path), "lerp" the straight line.  The path is deterministic: no eps is drawn and
    the ops stream does not move.  The decoder runs on chunks of fractions (`sample_chunks`; `chunk` lowers the chunk size); a
    latent does not depend on the chunking.  debug: frames as fp32 clamped to [0, 1], "coef" (P, T, 2), the path coefficients
    that were used, and "latents" (P, T, C, h, w)."""
    frames = _as_frames(frames)
    n, h, w, _ = frames.shape
    sampler_of(model, architecture, direction)                      # refusals come before anything is copied
    _check_interpolation(steps, mode)
    if n < 2:
        raise ValueError(f"interpolate: a path needs two frames, got {n}")
    ops.check_translate_size(n, h, w)
    device = device or next(model.parameters()).device
    x, window = ops.image_load(frames.to(device, non_blocking=True))
    return interpolate_padded(model, architecture, x, window, steps, direction, mode, chunk, debug)


def unevenness(step_l1):
    """max / mean of a pair's steps: 1 for a path whose decoded frames move evenly, large where it jumps; None when the mean is 0
    (nothing moved) or a step is not finite."""
    steps = [float(v) for v in step_l1]
    if not steps or not all(math.isfinite(v) for v in steps):
        return None
    mean = sum(steps) / len(steps)
    return max(steps) / mean if mean > 0 else None


def interpolation_output_names(paths, steps):
    """[(file name, input index i, fraction j)] in path order: <stem(i)>_i00.png is input i itself (fraction 0 of the pair it
    opens; the last input: the end of the pair it closes), <stem(i)>_i01.png ... the `steps` frames between it and the next
    input.  A sorted listing of the names of sorted stems is the path: len(paths) + (len(paths) - 1) * steps pictures."""
    width = max(2, len(str(steps)))
    last = len(paths) - 1
    return [(f"{Path(p).stem}_i{j:0{width}d}.png", i, j) for i, p in enumerate(paths) for j in range(1 if i == last else steps + 1)]


def interpolation_windows(n, batch_size):
    """[(start, stop, pairs)]: the encoder batches frames[start:stop] of a folder of n frames, at most `batch_size` each, and the
    pairs (i, i + 1) each decodes.  Every window but the first is handed the latent of the frame before it, so every frame is
    in exactly one batch and every consecutive pair in exactly one window."""
    if n < 1 or batch_size < 1:
        raise ValueError(f"interpolation_windows: n={n}, batch_size={batch_size}")
    return [(s, min(s + batch_size, n), [(i, i + 1) for i in range(max(s - 1, 0), min(s + batch_size, n) - 1)])
            for s in range(0, n, batch_size)]


def interpolation_record(name_a, name_b, omega, norm_a, norm_b, step_l1):
    """One pair's entry of metrics.json."""
    return {"a": name_a, "b": name_b, "omega": _finite_or_none(float(omega)), "norm_a": _finite_or_none(float(norm_a)),
            "norm_b": _finite_or_none(float(norm_b)), "step_l1": [_finite_or_none(float(v)) for v in step_l1],
            "unevenness": unevenness(step_l1)}


def check_interpolation_args(args):
    """The refusals of --interpolate that need nothing but the command line."""
    if args.interpolate < 1:
        raise ValueError(f"--interpolate must be at least 1 (intermediate frames between two inputs), got {args.interpolate}")
    if args.samples > 1:
        raise ValueError("--interpolate walks between the latent means of two frames: it cannot be combined with --samples (draws around one frame)")
    if args.targets:
        raise ValueError("--interpolate cannot be combined with --targets: the frames between two inputs have no expected image")


def check_interpolation_inputs(paths, shapes, batch_size, steps):
    """The refusals of --interpolate that need the list of inputs and their sizes ((H, W, C) each), before a model is loaded."""
    if len(paths) < 2:
        raise ValueError(f"--interpolate needs at least two inputs to walk between, found {len(paths)}")
    for p, s in zip(paths[1:], shapes[1:]):
        if tuple(s[:2]) != tuple(shapes[0][:2]):
            raise ValueError(f"--interpolate: all frames of a run must have one size, but {Path(paths[0]).name} is {shapes[0][0]}x{shapes[0][1]} "
                             f"and {Path(p).name} is {s[0]}x{s[1]}; use --size S to resize every frame to S x S")
        if tuple(s) != tuple(shapes[0]):
            raise ValueError(f"--interpolate: {Path(paths[0]).name} decodes to {shapes[0][2]} channel(s) and {Path(p).name} to {s[2]}; "
                             f"convert them to one mode")
    h, w = shapes[0][:2]
    if h < ops.MIN_TRANSLATE_SIDE or w < ops.MIN_TRANSLATE_SIDE:
        raise ValueError(f"--interpolate: the {h}x{w} frames are smaller than {ops.MIN_TRANSLATE_SIDE} on a side")
    hp, wp, _, _ = ops.pad_plan(h, w)
    try:
        sample_chunks(min(batch_size, len(paths)), hp, wp, steps + 2)
    except ValueError:
        raise ValueError(f"--interpolate {steps}: the {steps + 2} frames of a pair are decoded in chunks of whole windows, and one window of "
                         f"{min(batch_size, len(paths))} x {hp}x{wp} padded pixels exceeds the bound of {ops.MAX_TRANSLATE_PIXELS} per "
                         f"batch: use a smaller --batch_size or --size") from None


# ------------------------------------------------------------------ files
def discover_inputs(path):
    """The image files of `path` (one file, or the files of a directory in name order)."""
    p = Path(path)
    if p.is_file():
        return [p]
    if not p.is_dir():
        raise FileNotFoundError(f"--input {path}: no such file or directory")
    return sorted(f for f in p.iterdir() if f.is_file() and f.suffix.lower() in IMAGE_SUFFIXES)


def _mode_channels(mode):
    return {"L": 1, "RGB": 3, "RGBA": 4}.get(mode, 3)


def probe(path):
    """(H, W, C) a file will decode to, from its header."""
    from PIL import Image
    with Image.open(path) as im:
        return im.height, im.width, _mode_channels(im.mode)


def decode(path, channels=None):
    """uint8 (H, W, C): grey stays 1 channel, RGB 3, RGBA 4; every other mode is converted to RGB."""
    from PIL import Image
    with Image.open(path) as im:
        if channels == 3 and im.mode != "RGB" or im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGB")
        a = np.asarray(im)
    return a[:, :, None] if a.ndim == 2 else a


def group_by_size(paths, shapes, batch_size):
    """Batches of at most `batch_size` files of one decoded shape, in order of first appearance: [(shape, [paths])]."""
    by_shape = {}
    for p, s in zip(paths, shapes):
        by_shape.setdefault(tuple(s), []).append(p)
    return [(s, ps[i:i + batch_size]) for s, ps in by_shape.items() for i in range(0, len(ps), batch_size)]


def size_problem(n, h, w):
    """Why a batch of n frames of h x w cannot be translated, or None."""
    if h < ops.MIN_TRANSLATE_SIDE or w < ops.MIN_TRANSLATE_SIDE:
        return f"smaller than {ops.MIN_TRANSLATE_SIDE} on a side"
    hp, wp, _, _ = ops.pad_plan(h, w)
    if n * hp * wp > ops.MAX_TRANSLATE_PIXELS:
        return (f"{n} x {hp}x{wp} padded pixels exceed the bound of {ops.MAX_TRANSLATE_PIXELS} per batch (no tiling: InstanceNorm "
                f"statistics are per whole image)")
    return None


def output_name(path, suffix="_translated"):
    return f"{Path(path).stem}{suffix}.png"


def sample_output_names(path, samples, suffix="_translated"):
    """The PNGs --samples K writes for one input: the K draws, their mean, the spread map."""
    stem = f"{Path(path).stem}{suffix}"
    return {"samples": [f"{stem}_s{j:02d}.png" for j in range(samples)], "mean": f"{stem}_mean.png", "spread": f"{stem}_spread.png"}


def checkpoint_architecture(checkpoint_or_run_dir, architecture=None):
    """The architecture `load_generator` will build, without loading anything but a run directory's args.json."""
    path = Path(checkpoint_or_run_dir)
    if architecture is None and path.is_dir():
        with open(path / "args.json") as f:
            architecture = json.load(f)["architecture"]
    if architecture is None:
        raise ValueError("a bare checkpoint file needs --architecture (a run directory has it in args.json)")
    return train.ALIASES.get(architecture, architecture)


def build_parser():
    p = argparse.ArgumentParser(description="Translate whole images of any size with a trained generator (MI355X-native path)")
    p.add_argument("--checkpoint", required=True, help="a run directory (args.json + best_model.pth) or a .pth file")
    p.add_argument("--input", required=True, help="an image file or a directory of images")
    p.add_argument("--output", required=True, help="directory the PNGs (and metrics.json) are written to")
    p.add_argument("--architecture", type=str, default=None, choices=train.REFERENCE_ARCHS + list(train.ALIASES),
                   help="needed with a bare .pth; overrides args.json otherwise")
    p.add_argument("--latent_dim", type=int, default=None)
    p.add_argument("--direction", choices=["a2b", "b2a"], default="a2b",
                   help="a2b: G; b2a: F of the cycle models.  doubleae / doublevae: translate_A_to_B (decoder_B) / translate_B_to_A "
                        "(decoder_A) — not the reconstruction test.py shows for them")
    p.add_argument("--eps", choices=["sample", "mean"], default="sample",
                   help="variational generators: sample the latent (as test.py does) or decode its mean (deterministic)")
    p.add_argument("--seed", type=int, default=1234, help="the eps stream of --eps sample")
    p.add_argument("--samples", type=int, default=1,
                   help="variational generators: draw this many translations per frame from one encoder pass and write "
                        "<stem><suffix>_s00.png ..., their mean <stem><suffix>_mean.png and the per-pixel spread <stem><suffix>_spread.png "
                        "(grey).  1: one image per frame, as without the flag")
    p.add_argument("--temperature", type=float, default=1.0,
                   help="with --samples: scale of the latent noise, z = mu + T * eps * sigma (0 decodes the mean K times)")
    p.add_argument("--spread_gain", type=float, default=2.0,
                   help="with --samples: the spread PNG shows min(1, G * s).  The sample standard deviation s of K values in [0, 1] "
                        "cannot exceed 0.5 sqrt(K / (K - 1)), so the default 2 saturates only near that theoretical maximum: it is "
                        "derived, not tuned on a model, and a real model's maps are far darker — you will usually raise it")
    p.add_argument("--interpolate", type=int, default=None, metavar="N",
                   help="variational generators: write N frames between each two consecutive inputs (in name order), decoded from a "
                        "path between the two frames' latent means: <stem>_i00.png is the input's own translation, <stem>_i01.png ... "
                        "the frames towards the next input.  All frames must have one size (or use --size)")
    p.add_argument("--interp_mode", choices=list(ops.LATENT_PATH_MODES), default="slerp",
                   help="with --interpolate: slerp walks the great circle between the two latents, lerp the straight line")
    p.add_argument("--batch_size", type=int, default=1, help="frames of equal size are translated together, at most this many")
    p.add_argument("--size", type=int, default=None,
                   help="first resize every frame to SIZE x SIZE (the reference's Resize((S, S)); a multiple of 16, at least 32)")
    p.add_argument("--targets", type=str, default=None,
                   help="directory with the expected images under the same file names: writes metrics.json (L1, MSE, PSNR, SSIM)")
    p.add_argument("--ema", action="store_true", help="use the checkpoint's averaged generator weights (a run trained with --ema_decay)")
    p.add_argument("--suffix", type=str, default="_translated")
    p.add_argument("--num_workers", type=int, default=4, help="host threads that decode and write images")
    return p


class _PairFiles:
    """input_pipeline source over (input, target-or-input) files, for --size."""

    def __init__(self, paths, targets):
        self.paths, self.targets, self.paired = paths, targets, True

    def __len__(self):
        return len(self.paths)

    def pair(self, idx, rng):
        x = decode(self.paths[idx], 3)
        return x, (decode(self.targets[idx], 3) if self.targets else x)


def _pinned(shape):
    return torch.empty(shape, dtype=torch.uint8, pin_memory=torch.cuda.is_available())


def load_batch(paths, shape, pool):
    """The files of one batch decoded on the pool's threads into one pinned uint8 (N, H, W, C) buffer."""
    buf = _pinned((len(paths),) + tuple(shape))
    view = buf.numpy()

    def one(k):
        a = decode(paths[k])
        if a.shape != tuple(shape):
            raise ValueError(f"{paths[k]}: decoded to {a.shape}, its header said {tuple(shape)}")
        view[k] = a
    list(pool.map(one, range(len(paths))))
    return buf


def run_batch(model, architecture, frames, targets, args, device):
    """One batch on the device: (uint8 (N, H, W, 3) host array of the translated frames, (N, 4) float64 metrics or None)."""
    y, window = translate_padded(model, architecture, frames, args.direction, args.eps, None, device)
    metrics = None
    if targets is not None:
        t, _ = ops.image_load(targets.to(device, non_blocking=True))
        metrics = ops.image_metrics_hw(y, t, window).cpu().double().numpy()
    return ops.to_display_hw(y, window, uint8=True).cpu().numpy(), metrics


def run_resized(model, architecture, paths, targets, args, device):
    """--size: yields (paths of a batch, uint8 results, metrics) with every frame resized to S x S by the evaluator's pipeline."""
    pipe = input_pipeline.DeviceInputPipeline(_PairFiles(paths, targets), args.batch_size, args.size, device, recipe="test",
                                              shuffle=False, seed=args.seed, num_workers=max(1, args.num_workers),
                                              same_xy=targets is None)
    done = 0
    for batch in pipe:
        x = batch["x"]
        y = run_generator(model, architecture, x, args.direction, args.eps, None)
        metrics = ops.image_metrics_hw(y, batch["y"]).cpu().double().numpy() if targets is not None else None
        yield paths[done:done + x.shape[0]], ops.to_display_hw(y, None, uint8=True).cpu().numpy(), metrics
        done += x.shape[0]


def _sampled_to_host(res, names):
    """One batch of sample_padded on the host: per file (uint8 images, metric rows or None, mean spread)."""
    u8 = {k: res[k].cpu().numpy() for k in ("samples", "mean", "spread_u8")}
    spread = res["mean_spread"].cpu().double().numpy()
    rows = res["metrics"].cpu().double().numpy() if "metrics" in res else None
    srows = res["sample_metrics"].cpu().double().numpy() if "metrics" in res else None
    return [dict(name=n, samples=u8["samples"][i], mean=u8["mean"][i], spread=u8["spread_u8"][i], mean_spread=float(spread[i]),
                 metrics=None if rows is None else rows[i], sample_metrics=None if srows is None else srows[i])
            for i, n in enumerate(names)]


def run_batch_sampled(model, architecture, frames, targets, args, device):
    """run_batch for --samples K: the batch's sample_padded result (the eps stream goes on where it is)."""
    x, window = ops.image_load(frames.to(device, non_blocking=True))
    t = ops.image_load(targets.to(device, non_blocking=True))[0] if targets is not None else None
    return sample_padded(model, architecture, x, window, args.samples, args.direction, args.temperature, spread_gain=args.spread_gain,
                         target=t)


def run_resized_sampled(model, architecture, paths, targets, args, device):
    """run_resized for --samples K: yields (paths of a batch, sample_padded result)."""
    pipe = input_pipeline.DeviceInputPipeline(_PairFiles(paths, targets), args.batch_size, args.size, device, recipe="test",
                                              shuffle=False, seed=args.seed, num_workers=max(1, args.num_workers),
                                              same_xy=targets is None)
    done = 0
    for batch in pipe:
        x = ops.to_nhwc(batch["x"])
        n, _, hp, wp = x.shape
        yield paths[done:done + n], sample_padded(model, architecture, x, (0, 0, hp, wp), args.samples, args.direction,
                                                  args.temperature, spread_gain=args.spread_gain,
                                                  target=ops.to_nhwc(batch["y"]) if targets is not None else None)
        done += n


def samples_report(files, with_metrics):
    """--samples K: metrics.json in its usual shape for the MEAN images, each file with the K draws' metrics under "samples" and
    its "mean_spread" (with --targets); otherwise samples.json with the mean spread per file."""
    if not with_metrics:
        return {"num_files": len(files), "per_file": {f["name"]: {"mean_spread": _finite_or_none(f["mean_spread"])} for f in files}}
    rep = metrics_report([f["name"] for f in files], [f["metrics"] for f in files])
    for f in files:
        rep["per_file"][f["name"]]["samples"] = [{k: _finite_or_none(float(r[i])) for i, k in enumerate(METRIC_NAMES)}
                                                 for r in f["sample_metrics"]]
        rep["per_file"][f["name"]]["mean_spread"] = _finite_or_none(f["mean_spread"])
    return rep


def _finite_or_none(v):
    return float(v) if math.isfinite(v) else None


def metrics_report(names, rows):
    """metrics.json: per file and mean; PSNR is null where MSE is 0 (as in test.py's summary.json)."""
    per_file = {n: {k: _finite_or_none(float(r[i])) for i, k in enumerate(METRIC_NAMES)} for n, r in zip(names, rows)}
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    mean = {k: _finite_or_none(float(a[:, i].mean())) if len(a) else None for i, k in enumerate(METRIC_NAMES)}
    return {"num_files": len(names), "mean": mean, "per_file": per_file}


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("this path has no CPU implementation: an MI355X is required")
    return torch.device("cuda", torch.cuda.current_device())


def run_interpolation(args):
    """--interpolate N: the whole run.  Everything that can be refused is refused before the model is loaded."""
    check_interpolation_args(args)
    arch = checkpoint_architecture(args.checkpoint, args.architecture)
    if arch not in VARIATIONAL:
        raise ValueError(f"--interpolate needs a variational checkpoint ({', '.join(VARIATIONAL)}); {arch} has no latent distribution to walk")
    paths = discover_inputs(args.input)
    if args.size is not None:
        shapes = [(args.size, args.size, 3)] * len(paths)
    else:
        shapes = [probe(p) for p in paths] if len(paths) >= 2 else []
    check_interpolation_inputs(paths, shapes, args.batch_size, args.interpolate)
    device = _device()
    model, architecture = load_generator(args.checkpoint, args.architecture, args.latent_dim, None, device, ema=args.ema)
    generator_of(model, architecture, args.direction)
    print("--interpolate: the path runs between the latent means, so --eps is not used and no noise is drawn")
    out_dir = Path(args.output)
    out_dir.mkdir(parents=True, exist_ok=True)
    steps, last = args.interpolate, len(paths) - 1
    name_of = {(i, j): name for name, i, j in interpolation_output_names(paths, steps)}
    records = []
    pool = ThreadPoolExecutor(max_workers=max(1, args.num_workers))

    def write(pair_list, res):
        from PIL import Image
        u8 = res["frames"].cpu().numpy()
        omega, norm_a, norm_b, step_l1 = (res[k].cpu().double().numpy() for k in ("omega", "norm_a", "norm_b", "step_l1"))
        jobs = []
        for idx, (i, nxt) in enumerate(pair_list):
            jobs += [(name_of[(i, j)], u8[idx, j]) for j in range(steps + 1)]
            if nxt == last:
                jobs.append((name_of[(last, 0)], u8[idx, steps + 1]))
            records.append(interpolation_record(paths[i].name, paths[nxt].name, omega[idx], norm_a[idx], norm_b[idx], step_l1[idx]))
            print(f"  {paths[i].name} -> {paths[nxt].name}: {name_of[(i, 0)]} .. {name_of[(i, steps)]}")
        list(pool.map(lambda job: Image.fromarray(job[1]).save(out_dir / job[0]), jobs))

    carry = None
    if args.size is not None:
        pipe = input_pipeline.DeviceInputPipeline(_PairFiles(paths, None), args.batch_size, args.size, device, recipe="test",
                                                  shuffle=False, seed=args.seed, num_workers=max(1, args.num_workers), same_xy=True)
        done = 0
        for batch in pipe:
            x = ops.to_nhwc(batch["x"])
            n, _, hp, wp = x.shape
            res = interpolate_padded(model, architecture, x, (0, 0, hp, wp), steps, args.direction, args.interp_mode, carry=carry)
            write([(i, i + 1) for i in range(max(done - 1, 0), done + n - 1)], res)
            carry, done = res["last_mu"], done + n
    else:
        for start, stop, pair_list in interpolation_windows(len(paths), args.batch_size):
            frames = load_batch(paths[start:stop], shapes[0], pool)
            x, window = ops.image_load(frames.to(device, non_blocking=True))
            res = interpolate_padded(model, architecture, x, window, steps, args.direction, args.interp_mode, carry=carry)
            write(pair_list, res)
            carry = res["last_mu"]
    pool.shutdown()
    report = out_dir / "metrics.json"
    with open(report, "w") as f:
        json.dump({"interpolation": {"mode": args.interp_mode, "steps": steps, "pairs": records}}, f, indent=2, allow_nan=False)
    print(f"Saved metrics to: {report}")
    print(f"Wrote {len(name_of)} frame(s) of {len(paths)} input(s) into {out_dir}")
    return 0


def main(argv=None):
    """Returns the exit code: 0, or 1 when some frame was skipped (too small, too large, unreadable, no target)."""
    args = build_parser().parse_args(argv)
    if args.batch_size < 1:
        raise ValueError("--batch_size must be at least 1")
    if args.size is not None and (args.size < ops.MIN_TRANSLATE_SIDE or args.size % 16):
        raise ValueError(f"--size must be a multiple of 16 and at least {ops.MIN_TRANSLATE_SIDE}")
    if args.interpolate is not None:
        return run_interpolation(args)
    if args.samples < 1:
        raise ValueError("--samples must be at least 1")
    if args.samples >= 2:
        if args.eps == "mean":
            raise ValueError("--samples draws from the latent distribution: it cannot be combined with --eps mean (the mean has no spread)")
        _check_sampling(args.samples, args.temperature)
        if not (math.isfinite(args.spread_gain) and args.spread_gain >= 0):
            raise ValueError(f"--spread_gain must be finite and >= 0, got {args.spread_gain}")
        arch = checkpoint_architecture(args.checkpoint, args.architecture)
        if arch not in VARIATIONAL:
            raise ValueError(f"--samples needs a variational checkpoint ({', '.join(VARIATIONAL)}); {arch} has nothing to sample")
    elif args.temperature != 1.0:
        raise ValueError("--temperature scales the draws of --samples K: it needs --samples of at least 2")
    device = _device()
    model, architecture = load_generator(args.checkpoint, args.architecture, args.latent_dim, None, device, ema=args.ema)
    generator_of(model, architecture, args.direction)               # a direction the model does not have: fail before any file
    paths = discover_inputs(args.input)
    if not paths:
        print(f"No images found under {args.input}")
        return 1
    out_dir = Path(args.output)
    out_dir.mkdir(parents=True, exist_ok=True)
    skipped, target_of = [], {}
    if args.targets:
        for p in list(paths):
            t = Path(args.targets) / p.name
            if t.is_file():
                target_of[p] = t
            else:
                skipped.append((p, f"no target {t}"))
                paths.remove(p)
    ops.manual_seed(args.seed)                                      # one eps stream over the whole folder
    names, rows, done = [], [], [0]
    pool = ThreadPoolExecutor(max_workers=max(1, args.num_workers))

    def write(batch_paths, u8, metrics):
        from PIL import Image
        list(pool.map(lambda k: Image.fromarray(u8[k]).save(out_dir / output_name(batch_paths[k], args.suffix)),
                      range(len(batch_paths))))
        if metrics is not None:
            names.extend(p.name for p in batch_paths)
            rows.extend(metrics)
        for p in batch_paths:
            print(f"  {p.name} -> {output_name(p, args.suffix)}")
        done[0] += len(batch_paths)

    sampled = []

    def write_sampled(batch_paths, res):
        from PIL import Image
        files = _sampled_to_host(res, [p.name for p in batch_paths])
        jobs = []
        for p, f in zip(batch_paths, files):
            out_names = sample_output_names(p, args.samples, args.suffix)
            jobs += list(zip(out_names["samples"], f["samples"])) + [(out_names["mean"], f["mean"]), (out_names["spread"], f["spread"])]
            print(f"  {p.name} -> {out_names['samples'][0]} .. {out_names['samples'][-1]}, {out_names['mean']}, {out_names['spread']}")
        list(pool.map(lambda job: Image.fromarray(job[1]).save(out_dir / job[0]), jobs))
        sampled.extend(files)
        done[0] += len(batch_paths)

    if args.size is not None:
        problem = size_problem(args.batch_size, args.size, args.size)
        if problem:
            raise ValueError(f"--size {args.size} with --batch_size {args.batch_size}: {problem}")
        targets = [target_of[p] for p in paths] if args.targets else None
        if args.samples >= 2:
            for batch_paths, res in run_resized_sampled(model, architecture, paths, targets, args, device):
                write_sampled(batch_paths, res)
        else:
            for batch_paths, u8, metrics in run_resized(model, architecture, paths, targets, args, device):
                write(batch_paths, u8, metrics)
    else:
        shapes = []
        for p in list(paths):
            try:
                shapes.append(probe(p))
            except Exception as e:                                  # not an image, truncated header: reported, the folder goes on
                skipped.append((p, f"unreadable: {e}"))
                paths.remove(p)
        for shape, batch_paths in group_by_size(paths, shapes, args.batch_size):
            problem = size_problem(len(batch_paths), shape[0], shape[1])
            if problem:
                skipped.extend((p, f"{shape[0]}x{shape[1]}: {problem}") for p in batch_paths)
                continue
            try:
                frames = load_batch(batch_paths, shape, pool)
                targets = None
                if args.targets:
                    targets = load_batch([target_of[p] for p in batch_paths], probe(target_of[batch_paths[0]]), pool)
                    if targets.shape[1:3] != frames.shape[1:3]:
                        raise ValueError(f"target is {targets.shape[1]}x{targets.shape[2]}, input {shape[0]}x{shape[1]}")
            except (OSError, ValueError) as e:
                skipped.extend((p, str(e)) for p in batch_paths)
                continue
            if args.samples >= 2:
                write_sampled(batch_paths, run_batch_sampled(model, architecture, frames, targets, args, device))
                continue
            u8, metrics = run_batch(model, architecture, frames, targets, args, device)
            write(batch_paths, u8, metrics)
    pool.shutdown()
    if args.targets or args.samples >= 2:
        report = out_dir / ("metrics.json" if args.targets else "samples.json")
        with open(report, "w") as f:
            json.dump(samples_report(sampled, bool(args.targets)) if args.samples >= 2 else metrics_report(names, rows), f, indent=2,
                      allow_nan=False)
        print(f"Saved metrics to: {report}")
    for p, why in skipped:
        print(f"Skipped {p}: {why}", file=sys.stderr)
    print(f"Translated {done[0]} file(s) into {out_dir}"
          + (f", skipped {len(skipped)}" if skipped else ""))
    return 1 if skipped else 0


if __name__ == "__main__":
    sys.exit(main())
