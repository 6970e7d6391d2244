#!/usr/bin/env python3
"""Numbers of DESIGN.md's "The gradient-matching loss": vcg_grad_loss_fwd / _bwd at 8 x 3 x 256^2 with 4 scales next to vcg_l1_fwd /
_bwd on the same tensors in the same run, the four entries alternated round by round, each against the bytes it must move at
6.3 TB/s; then ms / step of the cyclevaegan 256^2 batch-8 step with lambda_grad 0 and 0.5, alternated three times.

A kernel time is the median over 15 rounds of (HIP-event time of 20 back-to-back calls) / 20 after 3 warm-up rounds: what one
more call costs a stream that is already busy, which is how the step sees it.  Both forwards are two launches (tiles, final
sum).  Writes OUT/grad_loss_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/grad_loss_bench.py            # STEP=0: kernels only
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
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def timed_us(fn, calls=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def kernels(n, h, w, scales, rounds=15, warm=3):
    a = ops.as_phys(ops.rand_uniform((n, 3, h, w), dev, seed=1))
    b = ops.as_phys(ops.rand_uniform((n, 3, h, w), dev, seed=2))
    out = torch.empty((), dtype=torch.float32, device=dev)
    g = torch.ones((), dtype=torch.float32, device=dev)
    ga = torch.empty_like(a)
    ws = ops.workspace(max(lib.vcg_grad_loss_workspace(n, h, w, scales), lib.vcg_reduce_workspace(a.numel())), dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    npx = n * h * w * 16
    runs = [
        ("vcg_grad_loss_fwd", 2 * npx, lambda: lib.vcg_grad_loss_fwd(P(a), P(b), P(out), n, h, w, scales, P(ws), ws.numel() * 4, st)),
        ("vcg_l1_fwd", 2 * npx, lambda: lib.vcg_l1_fwd(P(a), P(b), P(out), a.numel(), n * 3 * h * w, P(ws), ws.numel() * 4, st)),
        ("vcg_grad_loss_bwd", 3 * npx, lambda: lib.vcg_grad_loss_bwd(P(a), P(b), P(g), P(ga), n, h, w, scales, st)),
        ("vcg_l1_bwd (ga only)", 3 * npx, lambda: lib.vcg_l1_bwd(P(a), P(b), P(g), P(ga), None, a.numel(), n * 3 * h * w, st)),
    ]
    for name, _, fn in runs:
        assert fn() == 0, lib.vcg_last_error()
    ts = {name: [] for name, _, _ in runs}
    for i in range(warm + rounds):                       # alternating: every round times each entry once
        for name, _, fn in runs:
            us = timed_us(fn)
            if i >= warm:
                ts[name].append(us)
    say(f"{n} x 3 x {h} x {w}, {scales} scales   (pitch-4 fp32: {npx / 1e6:.2f} MB per tensor)")
    say(f"  {'entry':24s} {'us / call':>10s} {'min .. max':>17s} {'bytes floor us':>15s} {'x bytes':>8s}")
    med = {}
    for name, nbytes, _ in runs:
        med[name] = statistics.median(ts[name])
        floor = nbytes / HBM * 1e6
        say(f"  {name:24s} {med[name]:10.2f} {min(ts[name]):8.2f} ..{max(ts[name]):7.2f} {floor:15.2f} {med[name] / floor:8.1f}")
    new, l1 = med["vcg_grad_loss_fwd"] + med["vcg_grad_loss_bwd"], med["vcg_l1_fwd"] + med["vcg_l1_bwd (ga only)"]
    say(f"  forward + backward: gradient matching {new:.2f} us, L1 {l1:.2f} us: x {new / l1:.2f}")
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
        m.configure_loss(lambda_grad=lam)
        models[lam] = m
    batch = {"x": ops.rand_uniform((8, 3, 256, 256), dev, seed=11), "y": ops.rand_uniform((8, 3, 256, 256), dev, seed=12)}
    say("cyclevaegan 256^2 batch 8 unpaired, ms / step (10 steps after 3 warm-up), lambda_grad 0 | 0.5 (4 scales), alternated")
    for rnd in range(3):
        r = {lam: step_ms(models[lam], batch) for lam in (0.0, 0.5)}
        say(f"  round {rnd}: {r[0.0]:7.2f} | {r[0.5]:7.2f}   (+{(r[0.5] / r[0.0] - 1) * 100:.2f} %)")


if __name__ == "__main__":
    say(f"# tools/grad_loss_bench.py on {torch.cuda.get_device_name(0)}")
    kernels(8, 256, 256, 4)
    if os.environ.get("STEP", "1") != "0":
        steps()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "grad_loss_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
