#!/usr/bin/env python3
"""Numbers of DESIGN.md's sections on the optional image losses ("The structural loss", "The gradient-matching loss", "Focal
frequency loss"): the term's vcg_<term>_loss_fwd / _bwd next to vcg_l1_fwd / _bwd on the same tensors in the same run, the four
entries alternated round by round; then ms / step of the cyclevaegan 256^2 batch-8 step with lambda_<term> 0 and 0.5, alternated
three times.  ssim and grad (4 scales) are set against the bytes they must move at 6.3 TB/s, freq (alpha 1) against the
157.3 TF fp32-MFMA peak, from the matrix products its two DFT entries execute, padded tiles included.  (The frequency term's
errors against float64 are printed by tests/test_gpu_freq_loss.py.)

A kernel time is the median over 15 rounds of (HIP-event time of 20 back-to-back calls) / 20 after 3 warm-up rounds: what one
more call costs a stream that is already busy, which is how the step sees it.  Writes OUT/<term>_loss_bench.txt (OUT defaults to
profiles_out) and prints the same.

swd (the sliced Wasserstein term, DESIGN.md "Sliced Wasserstein training loss") has no single forward / backward entry: its
stage calls are timed one by one through ops on the level-0 tensors of the same batch, then ops.swd_loss (3 levels) forward and
forward + backward, then the step with lambda_swd 0 and 1.

msssim (5 scales; DESIGN.md "The multi-scale structural loss") is set against ssim on the same box: its pyramid holds 4/3 of
level 0's pixels, so 4/3 of the structural loss's forward + backward plus the pooling traffic is the yardstick.  Its 2 x 2 pooling
is a kernel of its own between the levels' forward launches; the extra line prices it by vcg_swd_pool, the same pooling of ONE
image at level 0 (both images over all levels: about 2 x 4/3 of that), which is what fusing it into the forward could save.

    python tools/image_loss_bench.py <ssim|msssim|grad|freq|swd>        # STEP=0: kernels only
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
PEAK = 157.3e12       # fp32 MFMA, FLOP / s
TILE, CHUNK = 64, 32  # csrc/freq_loss.hip: FF_TM = FF_TN, FF_TK
SHAPES = {"ssim": [(8, 256, 256), (2, 32, 32)], "msssim": [(8, 256, 256)], "grad": [(8, 256, 256)], "freq": [(8, 256, 256)], "swd": [(8, 256, 256)]}
ON_WEIGHT = {"swd": 1.0}          # the weight of the "on" step; 0.5 for the others
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


def freq_flops(n, h, w):
    """One direction (forward and adjoint execute the same products): every workgroup runs whole 64 x 64 x 32 chunks, the row
    pass two real products per chunk (real operand, or real part only), the column pass four (complex x complex)."""
    up = lambda v, t: -(-v // t)  # noqa: E731
    row = up(3 * n * h, TILE) * up(w, TILE) * up(w, CHUNK) * 2
    col = 3 * n * up(h, TILE) * up(w, TILE) * up(h, CHUNK) * 4
    return (row + col) * 2.0 * TILE * TILE * CHUNK


def term_calls(term, a, b, out, g, ga, n, h, w, st):
    """-> (workspace bytes, forward call, backward call) of the term's two entries on the physical tensors."""
    if term == "ssim":
        return (lib.vcg_ssim_loss_workspace(n, h, w),
                lambda ws: lib.vcg_ssim_loss_fwd(P(a), P(b), P(out), n, h, w, P(ws), ws.numel() * 4, st),
                lambda ws: lib.vcg_ssim_loss_bwd(P(a), P(b), P(g), P(ga), n, h, w, st))
    if term == "msssim":                                   # the backward reads what the forward left in the workspace
        need = lib.vcg_msssim_loss_workspace(n, h, w, 5)   # ... so it is a buffer of the term's own, as in ops, not the shared one
        keep = torch.empty(need // 4, dtype=torch.float32, device=dev)
        return (need,
                lambda ws: lib.vcg_msssim_loss_fwd(P(a), P(b), P(out), n, h, w, 5, P(keep), need, st),
                lambda ws: lib.vcg_msssim_loss_bwd(P(a), P(b), P(g), P(ga), n, h, w, 5, P(keep), need, st))
    if term == "grad":
        return (lib.vcg_grad_loss_workspace(n, h, w, 4),
                lambda ws: lib.vcg_grad_loss_fwd(P(a), P(b), P(out), n, h, w, 4, P(ws), ws.numel() * 4, st),
                lambda ws: lib.vcg_grad_loss_bwd(P(a), P(b), P(g), P(ga), n, h, w, 4, st))
    keep = lib.vcg_freq_loss_spectrum(n, h, w)
    spec = torch.empty(keep // 4, dtype=torch.float32, device=dev)
    return (lib.vcg_freq_loss_workspace(n, h, w),
            lambda ws: lib.vcg_freq_loss_fwd(P(a), P(b), P(out), n, h, w, 1.0, P(spec), keep, P(ws), ws.numel() * 4, st),
            lambda ws: lib.vcg_freq_loss_bwd(P(spec), keep, P(g), P(ga), n, h, w, 1.0, P(ws), ws.numel() * 4, st))


def kernels(term, n, h, w, rounds=15, warm=3):
    a = ops.as_phys(ops.rand_uniform((n, 3, h, w), dev, seed=1))
    b = ops.as_phys(ops.rand_uniform((n, 3, h, w), dev, seed=2))
    out = torch.empty((), dtype=torch.float32, device=dev)
    g = torch.ones((), dtype=torch.float32, device=dev)
    ga = torch.empty_like(a)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need, fwd, bwd = term_calls(term, a, b, out, g, ga, n, h, w, st)
    ws = ops.workspace(max(need, lib.vcg_reduce_workspace(a.numel())), dev)
    npx = n * h * w * 16
    runs = [
        (f"vcg_{term}_loss_fwd", 2 * npx, lambda: fwd(ws)),
        ("vcg_l1_fwd", 2 * npx, lambda: lib.vcg_l1_fwd(P(a), P(b), P(out), a.numel(), n * 3 * h * w, P(ws), ws.numel() * 4, st)),
        (f"vcg_{term}_loss_bwd", 3 * npx, lambda: bwd(ws)),
        ("vcg_l1_bwd (ga only)", 3 * npx, lambda: lib.vcg_l1_bwd(P(a), P(b), P(g), P(ga), None, a.numel(), n * 3 * h * w, st)),
    ]
    if term == "msssim":
        runs.insert(2, ("vcg_swd_pool (1 image)", npx + npx // 4, lambda: lib.vcg_swd_pool(P(a), P(ga), n, h, w, st)))
    for name, _, fn in runs:
        assert fn() == 0, lib.vcg_last_error()
    ts = {name: [] for name, _, _ in runs}
    for i in range(warm + rounds):                       # alternating: every round times each entry once
        for name, _, fn in runs:
            us = timed_us(fn)
            if i >= warm:
                ts[name].append(us)
    say(f"{n} x 3 x {h} x {w}   (pitch-4 fp32: {npx / 1e6:.2f} MB per tensor, scratch {need / 1e6:.2f} MB)")
    say(f"  {'entry':24s} {'us / call':>10s} {'min .. max':>17s} {'bytes floor us':>15s} {'x bytes':>8s}")
    med = {}
    for name, nbytes, _ in runs:
        med[name] = statistics.median(ts[name])
        floor = nbytes / HBM * 1e6
        tail = f"{floor:15.2f} {med[name] / floor:8.1f}"
        if term == "freq" and "freq" in name:
            tf = freq_flops(n, h, w) / med[name] / 1e6
            tail = f"{freq_flops(n, h, w) / 1e9:.2f} GFLOP executed, {tf:.1f} TF, {tf * 1e12 / PEAK * 100:.1f}% of peak"
        say(f"  {name:24s} {med[name]:10.2f} {min(ts[name]):8.2f} ..{max(ts[name]):7.2f} {tail}")
    new, l1 = med[f"vcg_{term}_loss_fwd"] + med[f"vcg_{term}_loss_bwd"], med["vcg_l1_fwd"] + med["vcg_l1_bwd (ga only)"]
    say(f"  forward + backward: {term} {new:.2f} us, L1 {l1:.2f} us: x {new / l1:.2f}")
    if term == "msssim":
        pool = med["vcg_swd_pool (1 image)"] * 2 * 4 / 3
        say(f"  pooling, both images over all levels, about {pool:.2f} us = {pool / med['vcg_msssim_loss_fwd'] * 100:.1f} % of the forward")
    say()


def swd_kernels(n, h, w, rounds=15, warm=3):
    """The stages of one level (level 0: the largest), then the whole term over 3 levels."""
    loss = pkg.Losses.SlicedWassersteinLoss(levels=3, seed=1)
    a = ops.to_nhwc(ops.rand_uniform((n, 3, h, w), dev, seed=1))
    b = ops.to_nhwc(ops.rand_uniform((n, 3, h, w), dev, seed=2))
    ap, dirs = ops.as_phys(a), loss.directions(dev, 0)
    s = ops.swd_cell_side(n, h, w)
    desc = ops.swd_grid_gather(ap, s, 1, 0)
    proj = ops.swd_project(desc, dirs)
    keys, rows = ops.sort_columns_indexed(proj)
    other = ops.sort_columns(ops.swd_project(ops.swd_grid_gather(ops.as_phys(b), s, 1, 0), dirs))
    _, gproj, _ = ops.swd_pair_loss(keys, other, rows)
    gdesc = ops.swd_project(dirs, gproj).t()
    fine, coarse = torch.zeros_like(ap), ops.swd_pool(ap)
    g = torch.ones((), dtype=torch.float32, device=dev)
    nd = desc.shape[0]
    a_req = a.detach().clone().requires_grad_(True)

    def whole(backward):
        v = ops.swd_loss(a_req if backward else a, b, 3, ops.SwdPlan(loss.offsets(n, h, w, 0), dirs))
        if backward:
            a_req.grad = None
            v.backward()

    runs = [
        ("swd_pool", lambda: ops.swd_pool(ap)),
        ("swd_grid_gather", lambda: ops.swd_grid_gather(ap, s, 1, 0)),
        ("swd_project", lambda: ops.swd_project(desc, dirs)),
        ("sort_columns_indexed", lambda: ops.sort_columns_indexed(proj)),
        ("sort_columns", lambda: ops.sort_columns(proj)),
        ("swd_pair_loss", lambda: ops.swd_pair_loss(keys, other, rows)),
        ("swd_project (transposed)", lambda: ops.swd_project(dirs, gproj)),
        ("swd_grid_scatter", lambda: ops.swd_grid_scatter(gdesc, (n, h, w), s, 1, 0, 1.0 / nd, g)),
        ("swd_pool_adjoint_add", lambda: ops.swd_pool_adjoint_add(coarse, fine)),
        ("swd_loss forward, 3 levels", lambda: whole(False)),
        ("swd_loss fwd + bwd, 3 levels", lambda: whole(True)),
    ]
    ts = {name: [] for name, _ in runs}
    for i in range(warm + rounds):
        for name, fn in runs:
            us = timed_us(fn, calls=10)
            if i >= warm:
                ts[name].append(us)
    say(f"{n} x 3 x {h} x {w}: cells of {s}x{s}, {nd} descriptors per set on level 0, {dirs.shape[1]} directions")
    say(f"  {'stage (ops call, allocation included)':40s} {'us / call':>10s} {'min .. max':>17s}")
    for name, _ in runs:
        say(f"  {name:40s} {statistics.median(ts[name]):10.2f} {min(ts[name]):8.2f} ..{max(ts[name]):7.2f}")
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


def steps(term):
    models = {}
    on = ON_WEIGHT.get(term, 0.5)
    for lam in (0.0, on):
        torch.manual_seed(3)
        m = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).train()
        m.configure_optimizers(lr=2e-4)
        m.configure_loss(**{f"lambda_{term}": lam})
        models[lam] = m
    batch = {"x": ops.rand_uniform((8, 3, 256, 256), dev, seed=11), "y": ops.rand_uniform((8, 3, 256, 256), dev, seed=12)}
    say(f"cyclevaegan 256^2 batch 8 unpaired, ms / step (10 steps after 3 warm-up), lambda_{term} 0 | {on:g}, alternated")
    for rnd in range(3):
        r = {lam: step_ms(models[lam], batch) for lam in (0.0, on)}
        say(f"  round {rnd}: {r[0.0]:7.2f} | {r[on]:7.2f}   ({(r[on] / r[0.0] - 1) * 100:+.2f} %)")


if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in SHAPES:
        sys.exit(__doc__)
    term = sys.argv[1]
    say(f"# tools/image_loss_bench.py {term} on {torch.cuda.get_device_name(0)}")
    for shape in SHAPES[term]:
        if term == "swd":
            swd_kernels(*shape)
        else:
            kernels(term, *shape)
    if os.environ.get("STEP", "1") != "0":
        steps(term)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"{term}_loss_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
