#!/usr/bin/env python3
"""Numbers of DESIGN.md's "Feature matching": what the fused feature-matching op (csrc/feature_match.hip) costs on one
discriminator's activations at the headline shapes — batch 8 at 256 x 256: (8, 64, 128, 128), (8, 128, 64, 64), (8, 256, 32, 32),
(8, 512, 16, 16) — beside the same term composed from other ops, and what a cyclevaegan training step takes with the term.

Op time, forward + backward through autograd (ops.feature_matching(...).backward() against the composition's), both modes:
  pair  composed = ops.l1_loss per layer + ops.weighted_sum (nine launches forward, eight backward)
  mean  composed = torch's mean(dim=(0, 2, 3)), abs, mean on the logical views (no composition from the package's ops exists)
and the library calls alone (vcg_feature_match_fwd, vcg_feature_match_bwd), whose time over the bytes the algorithm moves — forward
reads both operands; backward reads both and writes one (pair) or writes one (mean) — is the achieved rate, set beside the 6.3 TB/s
a float4 copy reaches on this card (8 TB/s HBM3E peak).  A time is the median over 15 repetitions of (HIP-event time of 10
back-to-back calls) / 10 after 3 warm-up repetitions: launch-to-launch cost on one stream, the operands (126 MB) resident in the
256 MB Infinity Cache at best in part.  Fused and composed alternate.

Step time: cyclevaegan unpaired, batch 8, 256 x 256, latent 64, median of 10 steps after 4 warm-up steps, with lambda_fm = 0 (no
object is built and no launch made: the step of the commit before the term), lambda_fm = 10 in the mean mode, and 0 again.

Writes OUT/fm_loss_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/fm_bench.py
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
lines = []
SHAPES = [(8, 64, 128, 128), (8, 128, 64, 64), (8, 256, 32, 32), (8, 512, 16, 16)]
COPY_RATE = 6.3e12          # bytes/s of a float4 copy on the MI355X (8 TB/s HBM3E peak)


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def event_us(fn, calls=10, reps=15, warm=3):
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


def composed(mode):
    def pair(fakes, reals):
        terms = [ops.l1_loss(f, r) for f, r in zip(fakes, reals)]
        return ops.weighted_sum(terms, [1.0 / len(terms)] * len(terms))

    def mean(fakes, reals):
        terms = [(f.mean(dim=(0, 2, 3)) - r.mean(dim=(0, 2, 3))).abs().mean() for f, r in zip(fakes, reals)]
        return sum(terms) / len(terms)

    return {"pair": pair, "mean": mean}[mode]


def op_times():
    fakes = [ops.to_nhwc(ops.randn(s, dev, seed=31 + i)).detach().requires_grad_(True) for i, s in enumerate(SHAPES)]
    reals = [ops.to_nhwc(ops.randn(s, dev, seed=41 + i)).detach() for i, s in enumerate(SHAPES)]
    operand = sum(f.numel() for f in fakes) * 4
    n = len(SHAPES)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fp, rp = [ops.phys_of(f.detach()) for f in fakes], [ops.phys_of(r) for r in reals]
    grads = [torch.empty_like(p) for p in fp]

    def table(ts):
        return (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])

    rows = (ctypes.c_size_t * n)(*[s[0] * s[2] * s[3] for s in SHAPES])
    chans = (ctypes.c_int * n)(*[s[1] for s in SHAPES])
    out, up = torch.empty((), device=dev), torch.ones((), device=dev)
    signs = torch.empty(sum(ops.pitch(s[1]) for s in SHAPES), device=dev)
    say(f"one discriminator's activations at batch 8, 256 x 256: {operand / 1e6:.1f} MB per operand")
    for code, mode in enumerate(ops.FM_MODES):
        ws = torch.empty(lib.vcg_feature_match_workspace(rows, chans, n, code) // 4 + 4, device=dev)

        def lib_fwd():
            return lib.vcg_feature_match_fwd(table(fp), table(rp), rows, chans, n, code, out.data_ptr(), signs.data_ptr(),
                                             ws.data_ptr(), ws.numel() * 4, st)

        def lib_bwd():
            return lib.vcg_feature_match_bwd(table(fp), table(rp), signs.data_ptr(), up.data_ptr(), table(grads), rows, chans, n,
                                             code, st)

        def fused():
            for f in fakes:
                f.grad = None
            ops.feature_matching(fakes, reals, mode).backward()

        standin = composed(mode)

        def other():
            for f in fakes:
                f.grad = None
            standin(fakes, reals).backward()

        assert lib_fwd() == 0 and lib_bwd() == 0, lib.vcg_last_error()
        fused()
        g_fused = [f.grad.clone() for f in fakes]
        v_fused = ops.feature_matching(fakes, reals, mode).item()
        other()
        worst = max((a - f.grad).abs().max().item() / a.abs().max().item() for a, f in zip(g_fused, fakes))
        v_other = standin(fakes, reals).item()
        say(f"{mode}: value fused {v_fused!r}, composed {v_other!r}; gradients differ by at most {worst:.2e} of a layer's maximum")
        got = {}
        for name, fn in (("fused fwd + bwd (autograd)", fused), ("composed fwd + bwd (autograd)", other),
                         ("fused fwd + bwd (autograd), again", fused), ("composed fwd + bwd (autograd), again", other),
                         ("vcg_feature_match_fwd", lib_fwd), ("vcg_feature_match_bwd", lib_bwd)):
            got[name] = event_us(fn)
        moved = {"vcg_feature_match_fwd": 2 * operand, "vcg_feature_match_bwd": (3 if mode == "pair" else 1) * operand}
        say(f"  {'what':40s} {'us / call':>10s}")
        for name, us in got.items():
            rate = ""
            if name in moved:
                bps = moved[name] / (us * 1e-6)
                rate = f"   {moved[name] / 1e6:6.1f} MB -> {bps / 1e12:.2f} TB/s = {bps / COPY_RATE:.2f} of a float4 copy's rate"
            say(f"  {name:40s} {us:10.2f}{rate}")
        say(f"  composed / fused: {got['composed fwd + bwd (autograd)'] / got['fused fwd + bwd (autograd)']:.2f}"
            f" (again: {got['composed fwd + bwd (autograd), again'] / got['fused fwd + bwd (autograd), again']:.2f})")
        say()


def training_steps():
    torch.manual_seed(1234)
    batch = {"x": ops.rand_uniform((8, 3, 256, 256), dev, seed=1234, offset=0),
             "y": ops.rand_uniform((8, 3, 256, 256), dev, seed=1234, offset=1 << 22)}
    say("cyclevaegan unpaired, batch 8, 256 x 256, latent 64: ms per training step (median of 10 after 4 warm-up steps)")
    for name, kw in (("lambda_fm 0", {}), ("lambda_fm 10 mean", dict(lambda_fm=10.0, fm_mode="mean")), ("lambda_fm 0 (again)", {})):
        model = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).train()
        model.configure_optimizers(lr=2e-4)
        model.configure_loss(**kw)
        ops.manual_seed(7)
        ts = []
        for i in range(14):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = model.training_step(dict(batch))
            torch.cuda.synchronize()
            if i >= 4:
                ts.append((time.perf_counter() - t0) * 1e3)
        say(f"  {name:20s} {statistics.median(ts):8.3f} ms   (min {min(ts):.3f}, max {max(ts):.3f}; last G_loss {m['G_loss']:.4f}"
            + (f", loss_fm {m['loss_fm']:.5f}" if "loss_fm" in m else "") + ")")
        del model
        torch.cuda.empty_cache()
    say()


if __name__ == "__main__":
    say(f"# tools/fm_bench.py on {torch.cuda.get_device_name(0)}")
    op_times()
    training_steps()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "fm_loss_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
