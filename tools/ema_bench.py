#!/usr/bin/env python3
"""Numbers of DESIGN.md's "Averaged generator weights": what the extra pass of --ema_decay costs.

1. The kernels alone at the headline model's generator buffer (CycleVAEGAN, latent 64: F + G): vcg_ema_update (12 B per
   parameter), vcg_swap (16 B) and, as the yardstick from the same run, vcg_adam_step (28 B): us per call and achieved GB/s.  A
   kernel time is the median over 15 repetitions of (HIP-event time of 20 back-to-back calls) / 20 after 3 warm-up repetitions
   (tools/grad_clip_bench.py's method).
2. The headline training step (batch 8, 256 x 256, unpaired) with ema_decay off and on: two models in ONE process, timed in
   interleaved blocks off, on, off, on, ... of STEPS steps each (wall time between synchronisations); per pair the difference,
   and over the pairs the median and the spread of each side — the spread of the off blocks is the noise the difference has to
   be read against.

Writes OUT/ema_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/ema_bench.py [--pairs 6] [--steps 10] [--batch 8]
"""
import argparse
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


def generator_floats():
    """length of optimizer_G's flat buffer, from the module shapes (no device memory)"""
    with torch.device("meta"):
        m = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False)
    return sum((p.numel() + 3) // 4 * 4 for p in list(m.F.parameters()) + list(m.G.parameters()))      # optim._ALIGN


def kernels(n):
    g = ops.randn((n,), dev, seed=3) * 1e-3
    p = ops.randn((n,), dev, seed=4) * 0.05
    e = ops.randn((n,), dev, seed=5) * 0.05
    m = torch.zeros(n, dtype=torch.float32, device=dev)
    v = torch.zeros(n, dtype=torch.float32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc = (2e-4 / 0.5, 0.5, 0.999, 0.5, 0.001, 1e-8, 0.0316)
    runs = [
        ("vcg_adam_step", 28, lambda: lib.vcg_adam_step(P(p), P(g), P(m), P(v), n, *sc, 1.0, st)),
        ("vcg_ema_update", 12, lambda: lib.vcg_ema_update(P(e), P(p), n, 1e-3, None, st)),
        ("vcg_ema_update (w = 1)", 8, lambda: lib.vcg_ema_update(P(e), P(p), n, 1.0, None, st)),
        ("vcg_swap", 16, lambda: lib.vcg_swap(P(e), P(p), n, st)),
        ("vcg_adam_step (again)", 28, lambda: lib.vcg_adam_step(P(p), P(g), P(m), P(v), n, *sc, 1.0, st)),
    ]
    say(f"optimizer_G (F + G): {n} floats ({4 * n / 1e6:.1f} MB per buffer)")
    say(f"  {'entry':24s} {'B / param':>9s} {'us / call':>10s} {'GB/s':>8s}")
    got = {}
    for entry, per, fn in runs:
        assert fn() == 0, lib.vcg_last_error()
        us = kernel_us(fn)
        got[entry] = us
        say(f"  {entry:24s} {per:9d} {us:10.2f} {per * n / us / 1e3:8.0f}")
    share = got["vcg_ema_update"] / got["vcg_adam_step"]
    say(f"  ema / adam = {share:.3f} (bytes: 12 / 28 = {12 / 28:.3f}; {share / (12 / 28):.2f} x that share)   adam again / adam = "
        f"{got['vcg_adam_step (again)'] / got['vcg_adam_step']:.3f}")
    say()


def headline(pairs, steps, batch):
    def make(**kw):
        torch.manual_seed(0)
        model = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).train()
        model.configure_optimizers(lr=2e-4, **kw)
        model.configure_loss()
        return model

    models = {"off": make(), "on": make(ema_decay=0.999)}
    x = ops.rand_uniform((batch, 3, 256, 256), dev, seed=1234, offset=0)
    y = ops.rand_uniform((batch, 3, 256, 256), dev, seed=1234, offset=1 << 24)

    def block(model, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            model.training_step({"x": x, "y": y})
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for model in models.values():
        block(model, 3)                                      # warm-up: packs, workspaces, streams
    ms = {"off": [], "on": []}
    say(f"headline step: CycleVAEGAN unpaired, batch {batch}, 256 x 256, {pairs} interleaved pairs of {steps}-step blocks")
    say(f"  {'pair':>4s} {'off ms/step':>12s} {'on ms/step':>12s} {'on - off':>9s}")
    for k in range(pairs):
        for name in ("off", "on"):
            ms[name].append(block(models[name], steps))
        say(f"  {k:4d} {ms['off'][-1]:12.3f} {ms['on'][-1]:12.3f} {ms['on'][-1] - ms['off'][-1]:9.3f}")
    for name in ("off", "on"):
        say(f"  {name:3s}: median {statistics.median(ms[name]):.3f} ms/step, min {min(ms[name]):.3f}, max {max(ms[name]):.3f}")
    diffs = [b - a for a, b in zip(ms["off"], ms["on"])]
    say(f"  on - off: median {statistics.median(diffs):.3f} ms/step (pairs from {min(diffs):.3f} to {max(diffs):.3f}); "
        f"spread of the off blocks {max(ms['off']) - min(ms['off']):.3f} ms")
    with models["on"].ema_scope():
        pass                                                 # (the swap is exercised once: two launches and a pack rebuild)
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    say(f"# tools/ema_bench.py on {torch.cuda.get_device_name(0)}")
    kernels(generator_floats())
    headline(a.pairs, a.steps, a.batch)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "ema_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
