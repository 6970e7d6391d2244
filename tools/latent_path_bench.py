#!/usr/bin/env python3
"""Numbers of DESIGN.md's "Interpolating translator": the two kernels of csrc/latent_path.hip alone at the product's shapes, and
the same path written with eager torch ops on the device.

Latent maps of 64 x 16 x 16 (a 256 x 256 frame) and 64 x 64 x 64 (1024 x 1024), P = 1 and 7 pairs (a --batch_size 8 window),
T = 10 and 64 fractions, all T in one call (k = T).  Per entry: the median over 15 repetitions of (HIP-event time of 20
back-to-back calls) / 20 after 3 warm-up repetitions (tools/ema_bench.py's method), and the bytes the traffic model says a call
must move over that time:
  vcg_latent_pair_stats   2 P per floats read (+ the slots: not counted);
  vcg_latent_path         (2 + k) P per floats: a and b read once, k fractions written;
  torch                   the same (2 + k) P per floats, whatever the eager ops really move: the figure says how far the chain of
                          eager ops is from the model, not what its kernels achieve.
The working sets are a few MB to a few hundred MB: the smaller ones live in the caches between repetitions, so the rates of
those lines are cache rates, not HBM rates.  The torch path is the usual latent slerp in fp32 (sums, acos and sin in fp32), one
decoder batch (P, T, per) as the result; it is timed, not compared bit for bit.

Writes OUT/latent_path_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/latent_path_bench.py [--commit TEXT]
"""
import argparse
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
lines = []
SHAPES = [(64, 16, 16), (64, 64, 64)]
PAIRS = (1, 7)
FRACTIONS = (10, 64)


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


def torch_path(a, b, total, mode, out):
    """(P, per) fp32 maps -> out (P, T, per): the path in eager ops."""
    t = torch.linspace(0.0, 1.0, total, device=a.device).view(1, total, 1)
    if mode == "lerp":
        ca, cb = (1.0 - t).expand(a.shape[0], total, 1), t.expand(a.shape[0], total, 1)
    else:
        cos = ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).clamp(-1.0, 1.0)
        w = torch.acos(cos).view(-1, 1, 1)
        ca, cb = torch.sin((1.0 - t) * w) / torch.sin(w), torch.sin(t * w) / torch.sin(w)
    torch.add(ca * a[:, None], cb * b[:, None], out=out)
    return out


def one_shape(shape, pairs, total):
    c, h, w = shape
    per = h * w * ops.pitch(c)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mu = ops.randn((pairs + 1, per), dev, 7)                         # consecutive frames of one encoder batch: a = mu, b = mu + per
    a, b = mu[:-1], mu[1:]
    stats = torch.empty((pairs, 3), dtype=torch.float64, device=dev)
    nws = lib.vcg_latent_stats_workspace(pairs, per)
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    z = torch.empty((pairs, total, per), device=dev)
    zt = torch.empty((pairs, total, per), device=dev)
    path_bytes = 4 * per * pairs * (2 + total)
    runs = [
        ("vcg_latent_pair_stats", 4 * per * pairs * 2,
         lambda: lib.vcg_latent_pair_stats(P(a), P(b), P(stats), pairs, per, c, ops.pitch(c), P(ws), nws, st)),
        ("vcg_latent_path slerp", path_bytes,
         lambda: lib.vcg_latent_path(P(a), P(b), P(stats), P(z), None, pairs, total, 0, total, per, c, ops.pitch(c), 0, st)),
        ("vcg_latent_path lerp", path_bytes,
         lambda: lib.vcg_latent_path(P(a), P(b), None, P(z), None, pairs, total, 0, total, per, c, ops.pitch(c), 1, st)),
        ("torch slerp (eager, fp32)", path_bytes, lambda: 0 * len(torch_path(a, b, total, "slerp", zt))),
        ("torch lerp (eager, fp32)", path_bytes, lambda: 0 * len(torch_path(a, b, total, "lerp", zt))),
    ]
    say(f"latent {c} x {h} x {w} (per = {per}), P = {pairs}, T = k = {total}: z is {4 * per * pairs * total / 1e6:.2f} MB")
    say(f"  {'entry':30s} {'model MB':>9s} {'us / call':>10s} {'GB/s':>8s}")
    for entry, nbytes, fn in runs:
        assert fn() == 0, lib.vcg_last_error()
        us = kernel_us(fn)
        say(f"  {entry:30s} {nbytes / 1e6:9.2f} {us:10.2f} {nbytes / us / 1e3:8.0f}")
    lib.vcg_latent_path(P(a), P(b), P(stats), P(z), None, pairs, total, 0, total, per, c, ops.pitch(c), 0, st)
    torch_path(a, b, total, "slerp", zt)
    say(f"  max |kernel - torch| over z (slerp): {float((z - zt).abs().max()):.3e}")
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", type=str, default="(not given)", help="the commit of the tree that is measured, for the record")
    args = ap.parse_args()
    say(f"# tools/latent_path_bench.py on {torch.cuda.get_device_name(0)}; tree: {args.commit}")
    say("# us / call: median of 15 x (HIP-event time of 20 back-to-back calls / 20); GB/s: the (2 + k) P per traffic model (stats: 2 P per) over it")
    say()
    for shape in SHAPES:
        for pairs in PAIRS:
            for total in FRACTIONS:
                one_shape(shape, pairs, total)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "latent_path_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
