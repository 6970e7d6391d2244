#!/usr/bin/env python3
"""Numbers of DESIGN.md's "Adversarial objective": what one fused vcg_gan_terms_fwd + vcg_gan_terms_bwd (csrc/gan_terms.hip)
costs beside the four vcg_mse_const_fwd + vcg_mse_const_bwd pairs (csrc/misc.hip) that form the same four terms of one
discriminator's real / fake logits under LSGAN, and what a cyclevaegan training step takes under each objective.

Logit counts per side: 8, 8 x 4 and 8 x 289 — batch 8 at 256, 288 and 512 px (ops.head_output_shape).  The fused pair is timed
under all three objectives; its backward has all four upstream scalars set, as the four LSGAN backwards together have.  A time is
the median over 15 repetitions of (HIP-event time of 20 back-to-back calls) / 20 after 3 warm-up repetitions (tools/kl_bench.py's
method): back-to-back launches on one stream, so a figure is the launch-to-launch cost, not an isolated kernel's latency.  The
training step: cyclevaegan unpaired, batch 8, 256 x 256, latent 64, median of 10 steps after 4 warm-up steps, per objective,
lsgan measured again at the end.

Writes OUT/gan_terms_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/gan_terms_bench.py
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
COUNTS = [(8, "batch 8 at 256 px"), (8 * 4, "batch 8 at 288 px"), (8 * 289, "batch 8 at 512 px")]


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


def count(n, what):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    real, fake = ops.randn((n,), dev, seed=21) * 3.0, ops.randn((n,), dev, seed=22) * 3.0
    g_real, g_fake = torch.empty_like(real), torch.empty_like(fake)
    out6, out2 = torch.empty(6, device=dev), torch.empty(2, device=dev)
    ups = [torch.ones(1, device=dev) for _ in range(4)]
    table = (ctypes.c_void_p * 4)(*[u.data_ptr() for u in ups])

    def fused_fwd(code):
        return lib.vcg_gan_terms_fwd(P(real), n, P(fake), n, code, 0.0, P(out6), st)

    def fused_bwd(code):
        return lib.vcg_gan_terms_bwd(P(real), n, P(fake), n, code, 0.0, table, P(g_real), P(g_fake), st)

    def four_fwd():
        return [lib.vcg_mse_const_fwd(P(z), t, P(out2), n, st) for z, t in ((real, 0.0), (fake, 1.0), (real, 1.0), (fake, 0.0))]

    def four_bwd():
        return [lib.vcg_mse_const_bwd(P(z), t, P(ups[0]), P(g), n, st)
                for z, t, g in ((real, 0.0, g_real), (fake, 1.0, g_fake), (real, 1.0, g_real), (fake, 0.0, g_fake))]

    assert all(rc == 0 for rc in four_fwd() + four_bwd()), lib.vcg_last_error()
    assert all(fused_fwd(c) == 0 and fused_bwd(c) == 0 for c in range(3)), lib.vcg_last_error()
    torch.cuda.synchronize()
    runs = [("4 x mse_const fwd", four_fwd), ("4 x mse_const bwd", four_bwd), ("4 x mse_const fwd + bwd", lambda: (four_fwd(), four_bwd()))]
    for code, name in enumerate(ops.GAN_OBJECTIVES):
        runs += [(f"gan_terms {name} fwd", lambda c=code: fused_fwd(c)), (f"gan_terms {name} bwd", lambda c=code: fused_bwd(c)),
                 (f"gan_terms {name} fwd + bwd", lambda c=code: (fused_fwd(c), fused_bwd(c)))]
    runs.append(("4 x mse_const fwd + bwd (again)", lambda: (four_fwd(), four_bwd())))
    say(f"{n} logits per side ({what})")
    say(f"  {'what':34s} {'us / call':>10s}")
    got = {}
    for name, fn in runs:
        got[name] = kernel_us(fn)
        say(f"  {name:34s} {got[name]:10.2f}")
    four = got["4 x mse_const fwd + bwd"]
    say("  fused / four: " + ", ".join(f"{name} {got[f'gan_terms {name} fwd + bwd'] / four:.3f}" for name in ops.GAN_OBJECTIVES)
        + f"; four again / four = {got['4 x mse_const fwd + bwd (again)'] / four:.3f}")
    say()


def training_steps():
    torch.manual_seed(1234)
    batch = {"x": ops.rand_uniform((8, 3, 256, 256), dev, seed=1234, offset=0),
             "y": ops.rand_uniform((8, 3, 256, 256), dev, seed=1234, offset=1 << 22)}
    say("cyclevaegan unpaired, batch 8, 256 x 256, latent 64: ms per training step (median of 10 after 4 warm-up steps)")
    for name in ops.GAN_OBJECTIVES + ("lsgan",):
        model = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).train()
        model.configure_optimizers(lr=2e-4)
        model.configure_loss(gan_objective=name)
        ops.manual_seed(7)
        ts = []
        for i in range(14):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = model.training_step(dict(batch))
            torch.cuda.synchronize()
            if i >= 4:
                ts.append((time.perf_counter() - t0) * 1e3)
        say(f"  {name:10s} {statistics.median(ts):8.3f} ms   (min {min(ts):.3f}, max {max(ts):.3f}; last G_loss {m['G_loss']:.4f}, D_loss {m['D_loss']:.4f})")
        del model
        torch.cuda.empty_cache()
    say()


if __name__ == "__main__":
    say(f"# tools/gan_terms_bench.py on {torch.cuda.get_device_name(0)}")
    for n, what in COUNTS:
        count(n, what)
    training_steps()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "gan_terms_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
