#!/usr/bin/env python3
"""Numbers of DESIGN.md's "Image history pool": what --pool_size costs per training step.

The headline training step (CycleVAEGAN unpaired, batch 8, 256 x 256) on three models in ONE process, timed in interleaved blocks
off, filling, swapping, off, ... of STEPS steps each (wall time between synchronisations):

  off       no pool (the parent's step);
  filling   pools so large that they never fill during the run: every step is an identity step (one vcg_pool_exchange launch per
            pool that stores the batch; the D phase is the pool-less one);
  swapping  pools of one batch: full after the first step, so that (all but one step in 256 per pool) both discriminators take the
            extra pass on the exchanged batch.

Per round the differences to the off block, over the rounds the median and the spread of each side — the spread of the off blocks is
the noise the differences have to be read against.  Also the exchange launch alone at the step's size (HIP events, 20 calls).

Writes OUT/image_pool_bench.txt (OUT defaults to profiles_out) and prints the same.

    python tools/image_pool_bench.py [--rounds 6] [--steps 10] [--batch 8]
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
ops = pkg.ops
image_pool = importlib.import_module("vae-cyclegan-implementation_amd.image_pool")
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def exchange_alone(batch):
    fake = ops.to_nhwc(ops.rand_uniform((batch, 3, 256, 256), dev, seed=5, offset=0))
    say(f"vcg_pool_exchange alone, {batch} images of 256 x 256 x 4 floats (median of 15 x 20 calls):")
    for name, capacity in (("store (filling)", 4096), ("swap or keep (full)", batch)):
        pool = image_pool.ImagePool(capacity, 1)
        ts = []
        for i in range(18):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                pool.exchange(fake)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1) * 1e3 / 20)
        say(f"  {name:22s} {statistics.median(ts):8.2f} us / call (host planning and the output allocation included)")
    say()


def headline(rounds, steps, batch):
    def make(**kw):
        torch.manual_seed(0)
        model = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False).to(dev).train()
        model.configure_optimizers(lr=2e-4, **kw)
        model.configure_loss()
        return model

    never_full = (4 + rounds * steps) * batch + 1
    models = {"off": make(), "filling": make(pool_size=never_full, pool_seed=1), "swapping": make(pool_size=batch, pool_seed=1)}
    x = ops.rand_uniform((batch, 3, 256, 256), dev, seed=1234, offset=0)
    y = ops.rand_uniform((batch, 3, 256, 256), dev, seed=1234, offset=1 << 24)
    extra = {"filling": 0, "swapping": 0}

    def block(name, n):
        model = models[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            model.training_step({"x": x, "y": y})
            if name in extra:
                extra[name] += sum(not p.last_identity for p in model.image_pools.values())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for name in models:
        block(name, 3)                                       # warm-up: packs, workspaces, streams; "swapping" fills its pools
    extra.update(filling=0, swapping=0)
    ms = {name: [] for name in models}
    say(f"headline step: CycleVAEGAN unpaired, batch {batch}, 256 x 256, {rounds} interleaved rounds of {steps}-step blocks")
    say(f"  {'round':>5s} {'off ms/step':>12s} {'filling':>10s} {'swapping':>10s} {'fill - off':>11s} {'swap - off':>11s}")
    for k in range(rounds):
        for name in models:
            ms[name].append(block(name, steps))
        say(f"  {k:5d} {ms['off'][-1]:12.3f} {ms['filling'][-1]:10.3f} {ms['swapping'][-1]:10.3f} "
            f"{ms['filling'][-1] - ms['off'][-1]:11.3f} {ms['swapping'][-1] - ms['off'][-1]:11.3f}")
    for name in models:
        say(f"  {name:8s}: median {statistics.median(ms[name]):.3f} ms/step, min {min(ms[name]):.3f}, max {max(ms[name]):.3f}")
    for name in ("filling", "swapping"):
        diffs = [b - a for a, b in zip(ms["off"], ms[name])]
        say(f"  {name} - off: median {statistics.median(diffs):.3f} ms/step (rounds from {min(diffs):.3f} to {max(diffs):.3f}); "
            f"extra discriminator passes taken: {extra[name]} in {rounds * steps} steps")
    say(f"  spread of the off blocks {max(ms['off']) - min(ms['off']):.3f} ms")
    say(f"  memory: {never_full} and {batch} slots of 1 MiB per pool, two pools per model")
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    say(f"# tools/image_pool_bench.py on {torch.cuda.get_device_name(0)}")
    exchange_alone(a.batch)
    headline(a.rounds, a.steps, a.batch)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "image_pool_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
