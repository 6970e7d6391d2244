#!/usr/bin/env python3
"""Numbers of DESIGN.md's "KL control": what the free-bits floor costs beside the plain KL term.

Forward plus backward of the floored term (vcg_kl_fb_fwd + vcg_kl_fb_bwd, csrc/kl_free_bits.hip) and of the plain term
(vcg_kl_fwd + vcg_kl_bwd, csrc/misc.hip) on the same buffers in the same run, in the two latent shapes BASELINE.json uses:
(8, 64, 16, 16) and (16, 1024, 16, 16).  Both read mu and logvar once forward and once backward and write two gradients: 24 B per
latent value.  A time is the median over 15 repetitions of (HIP-event time of 20 back-to-back calls) / 20 after 3 warm-up
repetitions (tools/grad_clip_bench.py's method); forward and backward are also timed apart, and a launch that only writes four
floats (vcg_fill) gives the share of the difference that is launch latency: the floored forward has one launch more.

Writes OUT/kl_free_bits_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/kl_bench.py
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
lines = []
SHAPES = [(8, 64, 16, 16), (16, 1024, 16, 16)]
FLOOR = 0.5


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


def shape(n, c, h, w):
    rows, st = n * h * w, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mu = ops.randn((rows, c), dev, seed=11)
    lv = ops.randn((rows, c), dev, seed=12) * 0.5
    gmu, glv = torch.empty_like(mu), torch.empty_like(lv)
    g = torch.ones(1, device=dev)
    out3, klc, out1 = torch.empty(3, device=dev), torch.empty(c, device=dev), torch.empty(1, device=dev)
    ws_fb = torch.empty(lib.vcg_kl_fb_workspace(rows, c) // 4 + 4, device=dev)
    ws_pl = torch.empty(lib.vcg_reduce_workspace(rows * c) // 4 + 4, device=dev)
    one = torch.empty(4, device=dev)

    def fb_fwd():
        return lib.vcg_kl_fb_fwd(P(mu), P(lv), P(out3), P(klc), rows, c, c, FLOOR, P(ws_fb), ws_fb.numel() * 4, st)

    def fb_bwd():
        return lib.vcg_kl_fb_bwd(P(mu), P(lv), P(g), P(klc), P(gmu), P(glv), rows, c, c, FLOOR, st)

    def pl_fwd():
        return lib.vcg_kl_fwd(P(mu), P(lv), P(out1), rows * c, P(ws_pl), ws_pl.numel() * 4, st)

    def pl_bwd():
        return lib.vcg_kl_bwd(P(mu), P(lv), P(g), P(gmu), P(glv), rows * c, st)

    runs = [("plain fwd", pl_fwd), ("plain bwd", pl_bwd), ("plain fwd + bwd", lambda: (pl_fwd(), pl_bwd())),
            ("floored fwd", fb_fwd), ("floored bwd", fb_bwd), ("floored fwd + bwd", lambda: (fb_fwd(), fb_bwd())),
            ("plain fwd + bwd (again)", lambda: (pl_fwd(), pl_bwd())),
            ("one tiny launch (vcg_fill, 4 floats)", lambda: lib.vcg_fill(P(one), 0.0, 4, st))]
    assert fb_fwd() == 0 and fb_bwd() == 0 and pl_fwd() == 0 and pl_bwd() == 0, lib.vcg_last_error()
    torch.cuda.synchronize()
    nbytes = 24 * rows * c
    say(f"latent ({n}, {c}, {h}, {w}): {rows} rows x {c} channels, {nbytes / 1e6:.2f} MB moved per forward + backward; "
        f"plain KL {out1.item():.5f}, floored {out3[0].item():.5f}, {int(out3[2].item())} of {c} channels above the floor {FLOOR}")
    say(f"  {'what':38s} {'us / call':>10s}")
    got = {}
    for name, fn in runs:
        got[name] = kernel_us(fn)
        say(f"  {name:38s} {got[name]:10.2f}")
    pl, fb, tiny = got["plain fwd + bwd"], got["floored fwd + bwd"], got["one tiny launch (vcg_fill, 4 floats)"]
    say(f"  floored / plain = {fb / pl:.3f} ({fb - pl:+.2f} us); plain again / plain = {got['plain fwd + bwd (again)'] / pl:.3f}; "
        f"one launch is {tiny:.2f} us = {100 * tiny / max(fb - pl, 1e-9):.0f} % of the difference; "
        f"floored at {nbytes / fb / 1e3:.0f} GB/s, plain at {nbytes / pl / 1e3:.0f} GB/s")
    say()


if __name__ == "__main__":
    say(f"# tools/kl_bench.py on {torch.cuda.get_device_name(0)}")
    for s in SHAPES:
        shape(*s)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "kl_free_bits_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
