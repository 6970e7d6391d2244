#!/usr/bin/env python3
"""Numbers of DESIGN.md's "The structural loss": vcg_ssim_loss_fwd / _bwd at 8 x 3 x 256^2 and 2 x 3 x 32^2 next to vcg_l1_fwd /
_bwd on the same tensors, each against the bytes it must move at 6.3 TB/s and against the ~5 us launch floor of the emptiest
kernels; then ms / step of the cyclevaegan 256^2 batch-8 step with lambda_ssim 0 and 0.5, alternated three times.

A kernel time is the median over 15 repetitions of (HIP-event time of 20 back-to-back calls) / 20 after 3 warm-up repetitions:
what one more call costs a stream that is already busy, which is how the step sees it.  The forward is two launches (tiles,
final sum), as vcg_l1_fwd is.  Writes OUT/ssim_loss_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/ssim_loss_bench.py            # STEP=0: kernels only
"""
import ctypes
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("vae-cyclegan-implementation_amd")
ops, lib = pkg.ops, pkg._native.lib()
dev = torch.device("cuda:0")
HBM = 6.3e12          # practical bytes / s
LAUNCH_US = 5.0
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def kernel_us(fn, calls=20, reps=15, warm=3):
    ts = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    return statistics.median(ts)


def kernels(n, h, w):
    a = ops.as_phys(ops.rand_uniform((n, 3, h, w), dev, seed=1))
    b = ops.as_phys(ops.rand_uniform((n, 3, h, w), dev, seed=2))
    out = torch.empty((), dtype=torch.float32, device=dev)
    g = torch.ones((), dtype=torch.float32, device=dev)
    ga, gb = torch.empty_like(a), torch.empty_like(b)
    ws = ops.workspace(max(lib.vcg_ssim_loss_workspace(n, h, w), lib.vcg_reduce_workspace(a.numel())), dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    npx = n * h * w * 16
    runs = [
        ("vcg_ssim_loss_fwd", 2 * npx, lambda: lib.vcg_ssim_loss_fwd(P(a), P(b), P(out), n, h, w, P(ws), ws.numel() * 4, st)),
        ("vcg_ssim_loss_bwd", 3 * npx, lambda: lib.vcg_ssim_loss_bwd(P(a), P(b), P(g), P(ga), n, h, w, st)),
        ("vcg_l1_fwd", 2 * npx, lambda: lib.vcg_l1_fwd(P(a), P(b), P(out), a.numel(), n * 3 * h * w, P(ws), ws.numel() * 4, st)),
        ("vcg_l1_bwd (ga only)", 3 * npx, lambda: lib.vcg_l1_bwd(P(a), P(b), P(g), P(ga), None, a.numel(), n * 3 * h * w, st)),
    ]
    say(f"{n} x 3 x {h} x {w}   (pitch-4 fp32: {npx / 1e6:.2f} MB per tensor)")
    say(f"  {'entry':24s} {'us / call':>10s} {'bytes floor us':>15s} {'x bytes':>8s} {'x launch (5 us)':>16s}")
    for name, nbytes, fn in runs:
        assert fn() == 0, lib.vcg_last_error()
        us = kernel_us(fn)
        floor = nbytes / HBM * 1e6
        say(f"  {name:24s} {us:10.2f} {floor:15.2f} {us / floor:8.1f} {us / LAUNCH_US:16.1f}")
    say()


def step_ms(model, batch, steps=10, warm=3):
    for _ in range(warm):
        model.training_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.training_step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def steps():
    models = {}
    for lam in (0.0, 0.5):
        torch.manual_seed(3)
        m = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).train()
        m.configure_optimizers(lr=2e-4)
        m.configure_loss(lambda_ssim=lam)
        models[lam] = m
    batch = {"x": ops.rand_uniform((8, 3, 256, 256), dev, seed=11), "y": ops.rand_uniform((8, 3, 256, 256), dev, seed=12)}
    say("cyclevaegan 256^2 batch 8 unpaired, ms / step (10 steps after 3 warm-up), lambda_ssim 0 | 0.5, alternated")
    for rnd in range(3):
        r = {lam: step_ms(models[lam], batch) for lam in (0.0, 0.5)}
        say(f"  round {rnd}: {r[0.0]:7.2f} | {r[0.5]:7.2f}   (+{(r[0.5] / r[0.0] - 1) * 100:.2f} %)")


if __name__ == "__main__":
    say(f"# tools/ssim_loss_bench.py on {torch.cuda.get_device_name(0)}")
    kernels(8, 256, 256)
    kernels(2, 32, 32)
    if os.environ.get("STEP", "1") != "0":
        steps()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "ssim_loss_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
