#!/usr/bin/env python3
"""Numbers of DESIGN.md's "The translator": translate_images at 768x1024 (batch 1 and 4) against test.translate at the same pixel
counts in 256^2 frames (12 and 48), peak device memory, and a batch next to ops.MAX_TRANSLATE_PIXELS.  Medians of 10 timed calls
after 3 warm-up calls, each ended by a device synchronise.  Writes OUT/translate_timing.json (OUT defaults to profiles_out).

    python tools/translate_bench.py
    MODE=trace rocprofv3 --kernel-trace --stats -d OUT/trace -o tr --output-format csv -- python tools/translate_bench.py
    python tools/translate_trace_tables.py OUT/trace/tr_kernel_trace.csv      # per-kernel tables of the two workloads

MODE=trace is the short run for the profiler: three passes of the I/O kernels (one 768x1024 frame, 8 x 256^2), one large-frame
translation and one 12 x 256^2 test.translate."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("vae-cyclegan-implementation_amd")
tr = importlib.import_module("vae-cyclegan-implementation_amd.translate")
ev = importlib.import_module("vae-cyclegan-implementation_amd.test")
train = importlib.import_module("vae-cyclegan-implementation_amd.train")
ops = pkg.ops
dev = torch.device("cuda:0")
mode = os.environ.get("MODE", "time")
arch = "cyclevaegan"
torch.manual_seed(3)
model = train.create_model(arch, paired=False, latent_dim=64).to(dev).eval()
rng = np.random.RandomState(0)
big = {n: torch.from_numpy(rng.randint(0, 256, (n, 768, 1024, 3), dtype=np.uint8)).to(dev) for n in (1, 4)}
sq = {n: ops.image_load(torch.from_numpy(rng.randint(0, 256, (n, 256, 256, 3), dtype=np.uint8)).to(dev))[0] for n in (12, 48)}
tgt = {n: torch.from_numpy(rng.randint(0, 256, (n, 768, 1024, 3), dtype=np.uint8)).to(dev) for n in (1,)}
sq8 = torch.from_numpy(rng.randint(0, 256, (8, 256, 256, 3), dtype=np.uint8)).to(dev)

def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)

def io_pass(u8):
    x, win = ops.image_load(u8)
    ops.to_display_hw(x, win, uint8=True)
    ops.to_display_hw(x, win, uint8=False)
    ops.image_metrics_hw(x, x, win)

if mode == "trace":
    for _ in range(3):
        io_pass(big[1]); io_pass(sq8)
        tr.translate_images(model, arch, big[1], seed=1)
        ops.manual_seed(1); ev.translate(model, arch, sq[12])
    torch.cuda.synchronize()
    sys.exit(0)

out = {}
for n in (1, 4):
    torch.cuda.reset_peak_memory_stats()
    med, lo, hi = timed(lambda: tr.translate_images(model, arch, big[n], seed=1), 10)
    out[f"translate_images 768x1024 batch {n}"] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "frames_per_s": n / med,
        "Mpx_per_s": n * 0.786432 / med, "peak_alloc_MB": torch.cuda.max_memory_allocated() / 2**20,
        "ops_workspaces_MB": sum(t.numel() * t.element_size() for t in ops._WS.values() if isinstance(t, torch.Tensor)) / 2**20}
    print(json.dumps({f"big{n}": out[f"translate_images 768x1024 batch {n}"]}), flush=True)
for n in (12, 48):
    def f():
        ops.manual_seed(1); return ops.to_display(ev.translate(model, arch, sq[n]), uint8=True)
    med, lo, hi = timed(f, 10)
    out[f"test.translate 256x256 batch {n}"] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "frames_per_s": n / med, "Mpx_per_s": n * 0.065536 / med}
    print(json.dumps({f"sq{n}": out[f"test.translate 256x256 batch {n}"]}), flush=True)
# next to the bound: 10 frames of 768x1024 = 7,864,320 of 8,388,607 padded pixels; frames 0 and 9 against the batch-1 result
n = ops.MAX_TRANSLATE_PIXELS // (768 * 1024)
ten = big[1].expand(n, -1, -1, -1).contiguous()
torch.cuda.reset_peak_memory_stats()
a = tr.translate_images(model, arch, big[1], eps="mean", return_float=True)
b = tr.translate_images(model, arch, ten, eps="mean", return_float=True)
torch.cuda.synchronize()
out["near_bound"] = {"frames": n, "padded_pixels": n * 768 * 1024, "max_abs_diff_frame0_vs_batch1": float((b[0] - a[0]).abs().max()),
                     "max_abs_diff_last_vs_batch1": float((b[-1] - a[0]).abs().max()), "finite": bool(torch.isfinite(b).all()),
                     "peak_alloc_MB": torch.cuda.max_memory_allocated() / 2**20}
print(json.dumps(out["near_bound"]), flush=True)
OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles_out")
os.makedirs(OUT, exist_ok=True)
json.dump(out, open(os.path.join(OUT, "translate_timing.json"), "w"), indent=1)
