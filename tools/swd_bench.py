#!/usr/bin/env python3
"""Numbers of DESIGN.md's "Sliced Wasserstein distance": what the evaluator's SWD costs, at 128 images of 256 x 256.

  whole     SlicedWasserstein: add() of 16 batches of 8 (pyramids + gathers of both sets), then result() (normalise, project,
            sort, distance on 5 levels x 2 sets of 16384 descriptors), wall time between synchronisations;
  translate the yardstick for "cheap enough to be on by default": test.py's `translate` of the same 128 images through an
            untrained CycleVAEGAN generator, batches of 8, wall time;
  stages    each ops call alone at the 256-pixel level's size (HIP events, median of REPS calls);
  sort      `ops.sort_columns` beside `torch.sort(dim=0)` on the same (16384, 512) matrix, alternated call by call, in the
            transposed layout the pipeline uses and in row-major.

Writes OUT/swd_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/swd_bench.py [--images 128] [--batch 8] [--reps 7] [--commit <what to call this build>]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("vae-cyclegan-implementation_amd")
ops, swd = pkg.ops, pkg.swd
ev = importlib.import_module("vae-cyclegan-implementation_amd.test")
dev = torch.device("cuda:0")
lines = []
S = 256


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(ts):
    return f"median {statistics.median(ts):9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f}, {len(ts)} runs)"


def main(a):
    n, b = a.images, a.batch
    say(f"# tools/swd_bench.py on {torch.cuda.get_device_name(0)}, build: {a.commit}")
    say(f"# {n} images of {S} x {S} per set, batches of {b}, 128 patches per image and level = {n * swd.patches_for(n)} descriptors")
    fake = [ops.to_nhwc(ops.rand_uniform((b, 3, S, S), dev, seed=3, offset=i << 22)) for i in range(n // b)]
    real = [ops.to_nhwc(ops.rand_uniform((b, 3, S, S), dev, seed=4, offset=i << 22)) for i in range(n // b)]

    state = {}

    def add_all():
        sw = swd.SlicedWasserstein(S, n, 1)
        for f, r in zip(fake, real):
            sw.add(f, r)
        state["sw"] = sw

    def result():
        state["res"] = state["sw"].result()

    add_all(); result()                                      # warm-up
    t_add, t_res = wall(add_all, a.reps), wall(result, a.reps)
    say()
    say("whole SWD (wall time):")
    say(f"  add() x {n // b} batches        {fmt(t_add)}")
    say(f"  result()                 {fmt(t_res)}")
    total = statistics.median(t_add) + statistics.median(t_res)
    say(f"  total                    {total:9.3f} ms = {total / n:.3f} ms per image")
    say(f"  result: {state['res']}")

    torch.manual_seed(0)
    model = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).eval()
    ops.manual_seed(1)

    def translate_all():
        for f in fake:
            ev.translate(model, "cyclevaegan", f)

    translate_all()
    t_tr = wall(translate_all, a.reps)
    say()
    say("the evaluator's translate of the same images (CycleVAEGAN generator, eval mode, wall time):")
    say(f"  translate x {n // b} batches    {fmt(t_tr)}")
    ratio = total / statistics.median(t_tr)
    say(f"  SWD / translate = {ratio:.3f}: the SWD costs {'MORE than' if ratio > 1 else 'less than'} the translation it scores")
    del model

    sw = state["sw"]
    plan0 = sw.plans[0][:b * sw.patches_per_image]
    levels = ops.laplacian_pyramid(fake[0])
    desc = sw._desc[0][0]
    dirs = torch.from_numpy(sw.directions).to(dev)
    norm = ops.swd_normalize(desc)
    proj = ops.swd_project(norm, dirs)
    other = ops.sort_columns(ops.swd_project(ops.swd_normalize(sw._desc[0][1]), dirs))
    sorted_ = ops.sort_columns(proj)
    stages = [
        (f"laplacian_pyramid, {b} images (5 levels)", lambda: ops.laplacian_pyramid(fake[0])),
        (f"swd_gather, level 256, {len(plan0)} patches", lambda: ops.swd_gather(levels[0], plan0)),
        (f"swd_normalize ({desc.shape[0]}, 147)", lambda: ops.swd_normalize(desc)),
        (f"swd_project ({desc.shape[0]}, 147) x (147, 512)", lambda: ops.swd_project(norm, dirs)),
        (f"sort_columns ({desc.shape[0]}, 512)", lambda: ops.sort_columns(proj)),
        (f"swd_distance ({desc.shape[0]}, 512)", lambda: ops.swd_distance(sorted_, other)),
    ]
    say()
    say(f"stages alone (HIP events around one call, output allocation included; median of {a.reps}):")
    for name, fn in stages:
        fn()
        ts = [event_ms(fn) for _ in range(a.reps)]
        say(f"  {name:48s} {fmt(ts)}")
    flops = 2.0 * desc.shape[0] * 147 * 512
    tp = statistics.median([event_ms(stages[3][1]) for _ in range(a.reps)])
    say(f"  swd_project: {flops / tp / 1e9:.2f} TFLOP/s of fp32 products")

    say()
    say(f"sort_columns beside torch.sort(dim=0) on the same ({desc.shape[0]}, 512) matrix, alternated:")
    for label, m in (("transposed (the pipeline's layout)", proj), ("row-major", proj.contiguous())):
        ours, theirs = [], []
        ops.sort_columns(m); torch.sort(m, dim=0)
        for _ in range(a.reps):
            ours.append(event_ms(lambda: ops.sort_columns(m)))
            theirs.append(event_ms(lambda: torch.sort(m, dim=0)))
        assert torch.equal(ops.sort_columns(m), torch.sort(m, dim=0).values)
        say(f"  {label}")
        say(f"    ops.sort_columns  {fmt(ours)}")
        say(f"    torch.sort        {fmt(theirs)}")
        say(f"    sort_columns / torch.sort = {statistics.median(ours) / statistics.median(theirs):.3f}")

    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "swd_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commit", type=str, default="unknown")
    main(ap.parse_args())
