#!/usr/bin/env python3
"""Numbers of DESIGN.md's "Focal frequency loss": vcg_freq_loss_fwd / _bwd at 8 x 3 x 256^2 next to vcg_l1_fwd / _bwd on the
same tensors in the same run, the four entries alternated round by round, with the fraction of the 157.3 TF fp32-MFMA peak the
two DFT entries reach — from the matrix products they execute, padded tiles included; the errors against a float64 restatement
of the definition (torch.fft on the CPU) for the shapes of tests/test_gpu_freq_loss.py; then ms / step of the cyclevaegan 256^2
batch-8 step with lambda_freq 0 and 1, alternated three times.

A kernel time is the median over 15 rounds of (HIP-event time of 20 back-to-back calls) / 20 after 3 warm-up rounds: what one
more call costs a stream that is already busy, which is how the step sees it.  Writes OUT/freq_loss_bench.txt (OUT defaults to
profiles_out) and prints the same.

    python tools/freq_loss_bench.py            # STEP=0: kernels and errors only
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
PEAK = 157.3e12       # fp32 MFMA, FLOP / s
TILE, CHUNK = 64, 32  # csrc/freq_loss.hip: FF_TM = FF_TN, FF_TK
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


def executed_flops(n, h, w):
    """One direction (forward and adjoint execute the same products): every workgroup runs whole 64 x 64 x 32 chunks, the row
    pass two real products per chunk (real operand, or real part only), the column pass four (complex x complex)."""
    up = lambda v, t: -(-v // t)  # noqa: E731
    row = up(3 * n * h, TILE) * up(w, TILE) * up(w, CHUNK) * 2
    col = 3 * n * up(h, TILE) * up(w, TILE) * up(h, CHUNK) * 4
    return (row + col) * 2.0 * TILE * TILE * CHUNK


def kernels(n, h, w, alpha=1.0, rounds=15, warm=3):
    a = ops.as_phys(ops.rand_uniform((n, 3, h, w), dev, seed=1))
    b = ops.as_phys(ops.rand_uniform((n, 3, h, w), dev, seed=2))
    out = torch.empty((), dtype=torch.float32, device=dev)
    g = torch.ones((), dtype=torch.float32, device=dev)
    ga = torch.empty_like(a)
    need, keep = lib.vcg_freq_loss_workspace(n, h, w), lib.vcg_freq_loss_spectrum(n, h, w)
    ws = ops.workspace(max(need, lib.vcg_reduce_workspace(a.numel())), dev)
    spec = torch.empty(keep // 4, dtype=torch.float32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flops = executed_flops(n, h, w)
    runs = [
        ("vcg_freq_loss_fwd", flops, lambda: lib.vcg_freq_loss_fwd(P(a), P(b), P(out), n, h, w, alpha, P(spec), keep, P(ws), ws.numel() * 4, st)),
        ("vcg_l1_fwd", 0.0, lambda: lib.vcg_l1_fwd(P(a), P(b), P(out), a.numel(), n * 3 * h * w, P(ws), ws.numel() * 4, st)),
        ("vcg_freq_loss_bwd", flops, lambda: lib.vcg_freq_loss_bwd(P(spec), keep, P(g), P(ga), n, h, w, alpha, P(ws), ws.numel() * 4, st)),
        ("vcg_l1_bwd (ga only)", 0.0, lambda: lib.vcg_l1_bwd(P(a), P(b), P(g), P(ga), None, a.numel(), n * 3 * h * w, st)),
    ]
    for name, _, fn in runs:
        assert fn() == 0, lib.vcg_last_error()
    ts = {name: [] for name, _, _ in runs}
    for i in range(warm + rounds):                       # alternating: every round times each entry once
        for name, _, fn in runs:
            us = timed_us(fn)
            if i >= warm:
                ts[name].append(us)
    say(f"{n} x 3 x {h} x {w}, alpha {alpha:g}   (spectrum kept: {keep / 1e6:.2f} MB, scratch {need / 1e6:.2f} MB)")
    say(f"  {'entry':24s} {'us / call':>10s} {'min .. max':>17s} {'GFLOP executed':>15s} {'TF':>7s} {'of peak':>8s}")
    med = {}
    for name, fl, _ in runs:
        med[name] = statistics.median(ts[name])
        tf = fl / med[name] / 1e6
        tail = f"{fl / 1e9:15.2f} {tf:7.1f} {tf * 1e12 / PEAK * 100:7.1f}%" if fl else ""
        say(f"  {name:24s} {med[name]:10.2f} {min(ts[name]):8.2f} ..{max(ts[name]):7.2f} {tail}")
    new, l1 = med["vcg_freq_loss_fwd"] + med["vcg_freq_loss_bwd"], med["vcg_l1_fwd"] + med["vcg_l1_bwd (ga only)"]
    say(f"  forward + backward: focal frequency {new:.2f} us, L1 {l1:.2f} us")
    say()


def ref_value_and_grad(a, b, alpha):
    x = a.clone().requires_grad_(True)
    D = torch.fft.fft2(x - b, norm="ortho")
    p = D.real ** 2 + D.imag ** 2
    with torch.no_grad():
        m = torch.ones_like(p) if alpha == 0 else p ** (alpha / 2)
        top = m.amax(dim=(-2, -1), keepdim=True)
        w = torch.where(top > 0, m / torch.where(top > 0, top, torch.ones_like(top)), torch.zeros_like(m)).clamp(0.0, 1.0)
    loss = (w * p).mean()
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g


def errors():
    shapes = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 2, 3), (1, 3, 5), (3, 9, 17), (2, 16, 16), (2, 17, 33), (1, 31, 65), (1, 96, 40),
              (1, 130, 258), (1, 256, 256)]
    say("errors against float64 (torch.fft on the CPU), uniform(-1, 1) operands: loss relative | gradient max error / max |g|")
    say(f"  {'N x H x W':>14s} " + " ".join(f"{'alpha ' + str(al):>21s}" for al in (0.0, 0.5, 1.0)))
    for n, h, w in shapes:
        gen = torch.Generator().manual_seed(97 * n + 13 * h + w)
        a = (torch.rand((n, 3, h, w), generator=gen, dtype=torch.float64) * 2 - 1).float().double()
        b = (torch.rand((n, 3, h, w), generator=gen, dtype=torch.float64) * 2 - 1).float().double()
        cells = []
        for alpha in (0.0, 0.5, 1.0):
            ref, gref = ref_value_and_grad(a, b, alpha)
            x = a.float().to(dev).requires_grad_(True)
            loss = ops.freq_loss(x, b.float().to(dev), alpha)
            loss.backward()
            eg = (x.grad.cpu().double() - gref).abs().max().item() / gref.abs().max().item()
            cells.append(f"{abs(float(loss.detach()) - ref) / ref:9.1e} | {eg:9.1e}")
        say(f"  {f'{n} x {h} x {w}':>14s} " + " ".join(cells))
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
    for lam in (0.0, 1.0):
        torch.manual_seed(3)
        m = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).train()
        m.configure_optimizers(lr=2e-4)
        m.configure_loss(lambda_freq=lam)
        models[lam] = m
    batch = {"x": ops.rand_uniform((8, 3, 256, 256), dev, seed=11), "y": ops.rand_uniform((8, 3, 256, 256), dev, seed=12)}
    say("cyclevaegan 256^2 batch 8 unpaired, ms / step (10 steps after 3 warm-up), lambda_freq 0 | 1 (alpha 1), alternated")
    for rnd in range(3):
        r = {lam: step_ms(models[lam], batch) for lam in (0.0, 1.0)}
        say(f"  round {rnd}: {r[0.0]:7.2f} | {r[1.0]:7.2f}   ({(r[1.0] / r[0.0] - 1) * 100:+.2f} %)")


if __name__ == "__main__":
    say(f"# tools/freq_loss_bench.py on {torch.cuda.get_device_name(0)}")
    kernels(8, 256, 256)
    errors()
    if os.environ.get("STEP", "1") != "0":
        steps()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "freq_loss_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
