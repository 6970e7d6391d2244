"""Timings of the sliding discriminator head (csrc/patch_head.hip) -> profiles/patch_head_bench.txt.

Per kernel: the three launches vcg_patch_head_fwd / _dgrad / _wgrad at the head shapes of 512 x 512 (N = 8, 32 x 32 x 512 map) and
272 x 272 (N = 8, 17 x 17 x 512 map), beside torch.nn.functional.conv2d forward + its two gradients on the same tensors on the
same card, the two alternated round by round; the bytes each launch must move at least and the fraction of HBM bandwidth that
is.  Per step: ms / step of unpaired cyclevaegan at 512 x 512, batch 2, and the head's launches as a share of it.

    python tools/patch_head_bench.py [--rounds 20] [--out profiles/patch_head_bench.txt] [--no_step]
"""
import argparse
import importlib
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0            # MI355X peak HBM3E bandwidth, GB/s


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps       # us


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def kernels(pkg, dev, N, H, W, rounds, lines):
    lib, ops = pkg._native.lib(), pkg.ops
    C, KH, KW = 512, 16, 16
    OH, OW = H - KH + 1, W - KW + 1
    g_ = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(N, H, W, C, generator=g_).to(dev)
    wsn = (torch.randn(KH * KW * C, generator=g_) * 0.01).to(dev)
    g = torch.randn(N * OH * OW, generator=g_).to(dev)
    bias, sigma, u = torch.zeros(1, device=dev), torch.ones(1, device=dev), torch.ones(1, device=dev)
    v = torch.zeros(KH * KW * C, device=dev)
    out, dx = torch.empty(N * OH * OW, device=dev), torch.empty_like(x)
    gw, gb = torch.zeros(1, C, KH, KW, device=dev), torch.zeros(1, device=dev)
    nws = lib.vcg_patch_head_workspace(N, H, W, C, KH, KW)
    ws = torch.empty(nws // 4, device=dev)
    p, st = ops._ptr, ops._stream()
    ours = {
        "fwd": lambda: lib.vcg_patch_head_fwd(p(x), p(wsn), p(bias), p(out), N, H, W, C, KH, KW, p(ws), nws, st),
        "dgrad": lambda: lib.vcg_patch_head_dgrad(p(g), p(wsn), p(dx), N, H, W, C, KH, KW, st),
        "wgrad": lambda: lib.vcg_patch_head_wgrad(p(g), p(x), p(wsn), p(sigma), p(u), p(v), p(gw), p(gb), N, H, W, C, KH, KW,
                                                  p(ws), nws, st),
    }
    xt = x.permute(0, 3, 1, 2)                                        # NCHW view of the NHWC buffer (channels_last)
    wt = wsn.reshape(KH, KW, C).permute(2, 0, 1)[None].contiguous(memory_format=torch.channels_last)
    gt = g.reshape(N, 1, OH, OW)
    theirs = {
        "fwd": lambda: F.conv2d(xt, wt),
        "dgrad": lambda: torch.nn.grad.conv2d_input(xt.shape, wt, gt),
        "wgrad": lambda: torch.nn.grad.conv2d_weight(xt, wt.shape, gt),
    }
    for fn in list(ours.values()) + list(theirs.values()):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {("ours", k): [] for k in ours}
    t.update({("torch", k): [] for k in theirs})
    for _ in range(rounds):                                           # alternate the two sides round by round
        for k in ours:
            t[("ours", k)].append(timed(ours[k], 10))
        for k in theirs:
            t[("torch", k)].append(timed(theirs[k], 10))
    xb, wb = x.numel() * 4, wsn.numel() * 4
    least = {"fwd": xb + wb, "dgrad": xb + wb, "wgrad": xb + 2 * wb}
    lines.append(f"head N={N} map {H}x{W}x{C} -> {OH}x{OW} logits per image   ({rounds} alternated rounds of 10 launches, median us)")
    tot_o = tot_t = 0.0
    for k in ("fwd", "dgrad", "wgrad"):
        o, r = median(t[("ours", k)]), median(t[("torch", k)])
        tot_o, tot_t = tot_o + o, tot_t + r
        lines.append(f"  {k:6s} patch_head {o:9.1f} us   torch conv2d {r:9.1f} us   least bytes {least[k] / 1e6:6.1f} MB -> "
                     f"{least[k] / (o * 1e-6) / 1e9 / HBM_GBS * 100:5.1f} % of {HBM_GBS:.0f} GB/s")
    lines.append(f"  three  patch_head {tot_o:9.1f} us   torch conv2d {tot_t:9.1f} us   ratio {tot_o / tot_t:.2f}")
    return tot_o


def step(pkg, dev, lines):
    gan = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).train()
    gan.configure_optimizers(lr=2e-4)
    gan.configure_loss()
    xb = pkg.ops.rand_uniform((2, 3, 512, 512), dev, seed=1, offset=0)
    yb = pkg.ops.rand_uniform((2, 3, 512, 512), dev, seed=1, offset=1 << 22)
    for _ in range(3):
        gan.training_step({"x": xb, "y": yb})
    torch.cuda.synchronize()
    ms = timed(lambda: gan.training_step({"x": xb, "y": yb}), 10) / 1e3
    lines.append(f"cyclevaegan unpaired 512x512 batch 2: {ms:.2f} ms / step")
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_head_bench.txt"))
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    dev = torch.device("cuda:0")
    lines = [f"tools/patch_head_bench.py on {torch.cuda.get_device_name(0)}",
             "every sample is 10 back-to-back launches on the same tensors: the 16 MB map and the weight stay in L2 / Infinity Cache,",
             "so the times are warm-cache times on both sides (a fair comparison) and the '% of HBM' column sets a warm time against",
             "the HBM peak; inside a training step the map arrives cold, so the share of the step below is an estimate, not a measurement"]
    kernels(pkg, dev, 8, 32, 32, a.rounds, lines)
    kernels(pkg, dev, 8, 17, 17, a.rounds, lines)
    if not a.no_step:
        ms = step(pkg, dev, lines)
        lines_b2 = []
        head = kernels(pkg, dev, 2, 32, 32, a.rounds, lines_b2)       # the step's own head shape: batch 2
        # per step: 8 head forwards, 8 data gradients (4 in the G pass, 4 in the D pass) and 4 weight gradients at most; the
        # three-launch total times 8 over-counts the launches, but its times are warm-cache ones: an estimate
        lines.append(f"  head N=2 map 32x32x512: three launches {head:.1f} us; x 8 discriminator passes = "
                     f"{8 * head / 1e3:.3f} ms = {8 * head / 1e3 / ms * 100:.2f} % of the step (estimate from warm times)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
