#!/usr/bin/env python3
"""Numbers of DESIGN.md's "Gradient clipping": vcg_grad_norm, vcg_adam_step and vcg_adam_step_clipped at the flat buffer sizes of
the headline model's two optimizers (CycleVAEGAN, latent 64: F + G and DX + DY), each against the bytes it must move at 6.3 TB/s
(4 B per parameter for the norm, 28 B for Adam).

A kernel time is the median over 15 repetitions of (HIP-event time of 20 back-to-back calls) / 20 after 3 warm-up repetitions:
what one more call costs a stream that is already busy, which is how the step sees it (tools/image_loss_bench.py's method).  The
norm is two launches (chunks, final sum).  Writes OUT/grad_clip_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/grad_clip_bench.py
"""
import ctypes
import importlib
import os
import statistics
import sys

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


def flat_sizes():
    """the two optimizers' buffer lengths, from the module shapes (no device memory)"""
    with torch.device("meta"):
        m = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False)
    pad = lambda ps: sum((p.numel() + 3) // 4 * 4 for p in ps)      # noqa: E731  (optim._ALIGN)
    return {"optimizer_G (F + G)": pad(list(m.F.parameters()) + list(m.G.parameters())),
            "optimizer_D (DX + DY)": pad(list(m.DX.parameters()) + list(m.DY.parameters()))}


def kernels(name, n):
    g = ops.randn((n,), dev, seed=3) * 1e-3
    p = ops.randn((n,), dev, seed=4) * 0.05
    m = torch.zeros(n, dtype=torch.float32, device=dev)
    v = torch.zeros(n, dtype=torch.float32, device=dev)
    clip = torch.zeros(4, dtype=torch.float32, device=dev)
    ws = ops.grad_norm_workspace(n, dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc = (2e-4 / 0.5, 0.5, 0.999, 0.5, 0.001, 1e-8, 0.0316)
    runs = [
        ("vcg_grad_norm", 4 * n, lambda: lib.vcg_grad_norm(P(g), n, 1.0, 1.0, P(clip), P(ws), ws.numel() * 4, st)),
        ("vcg_adam_step", 28 * n, lambda: lib.vcg_adam_step(P(p), P(g), P(m), P(v), n, *sc, 1.0, st)),
        ("vcg_adam_step_clipped", 28 * n, lambda: lib.vcg_adam_step_clipped(P(p), P(g), P(m), P(v), n, *sc, 1.0, P(clip), st)),
        ("vcg_adam_step (again)", 28 * n, lambda: lib.vcg_adam_step(P(p), P(g), P(m), P(v), n, *sc, 1.0, st)),
    ]
    say(f"{name}: {n} floats ({4 * n / 1e6:.1f} MB per buffer)")
    say(f"  {'entry':24s} {'us / call':>10s} {'bytes floor us':>15s} {'x bytes':>8s}")
    got = {}
    for entry, nbytes, fn in runs:
        assert fn() == 0, lib.vcg_last_error()
        us = kernel_us(fn)
        got[entry] = us
        floor = nbytes / HBM * 1e6
        say(f"  {entry:24s} {us:10.2f} {floor:15.2f} {us / floor:8.2f}")
    say(f"  norm / adam = {got['vcg_grad_norm'] / got['vcg_adam_step']:.3f}   clipped / plain = "
        f"{got['vcg_adam_step_clipped'] / got['vcg_adam_step']:.3f}   plain again / plain = "
        f"{got['vcg_adam_step (again)'] / got['vcg_adam_step']:.3f}")
    say()


if __name__ == "__main__":
    say(f"# tools/grad_clip_bench.py on {torch.cuda.get_device_name(0)}")
    for name, n in flat_sizes().items():
        kernels(name, n)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "grad_clip_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
