#!/usr/bin/env python3
"""Evaluation of trained runs with the reference's `test.py` CLI: every run under --runs_dir with an `args.json` and a
`best_model.pth` is loaded in eval mode, translates its held-out images, and the comparison figures, per-model grids and a
`summary.json` per dataset / modality group are written to <output_dir>/test_results_<timestamp>/<dataset>/<modality>/.

Kept from the reference (test.py:31-70, 457-468, 583-600, 607-726): the flags and their defaults, run discovery, the grouping
(dataset type, legacy `paired` / `unpaired` = hypersim, then `<source>_to_<target>`), the figure layouts and the summary keys.
Added: `--batch_size`, `--seed` (the summer2winter y draws and the VAE eps), `--save_images` (every G(x) as a PNG),
`--reference_split`, runs of `--dataset synthetic` (their own group, evaluated on the held-out stream train.py validates on),
per-image L1 / MSE / PSNR / SSIM against the target on the device (csrc/metrics.hip) for the paired groups, and for every
group, paired or not, the sliced Wasserstein distance between the set {G(x)} and the set {y} (swd.py, csrc/swd.hip; `--no_swd`
switches it off): the one number an unpaired run gets.

Deliberate differences from the reference:
  * the held-out set is the run's OWN: hypersim is split by `train.split_indices` from the run's --seed and --test_split, as
    train.py split it, where the reference's test.py splits with random_split(seed 42) (:193-196) while its train.py splits
    unseeded — it evaluates on images its models trained on.  `--reference_split` restores the seed-42 subset.  maps and
    summer2winter use their val / test directories as both do, with train.py's x = y for autoencoder / vae runs;
  * every test sample gets the deterministic Resize((S, S)) + ToTensor of the reference's three test loaders;
  * G(x) comes from the generator alone (`translate`), not from the whole composite forward (:310-312), which for CycleVAEGAN is
    6 VAE and 4 discriminator passes, fails for aegan / vaegan (their forward needs y) and indexes the batch for autoencoder;
  * models are evaluated one at a time (the reference keeps a whole group loaded), and only the images that go into a figure or
    a PNG are converted (on the device) and copied to the host.
"""
import argparse
import json
import math
import os
import sys
import time
from datetime import datetime
from pathlib import Path

import numpy as np
import torch

if __package__ in (None, ""):
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    ops, utils, input_pipeline, swd = _pkg.ops, _pkg.utils, _pkg.input_pipeline, _pkg.swd
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")
else:
    from . import input_pipeline, ops, swd, train, utils

GRID_SAMPLES = 8                                   # rows of a per-model grid (test.py:378)
METRIC_NAMES = ("l1", "mse", "psnr", "ssim")


def build_parser():
    p = argparse.ArgumentParser(description="Test and compare trained VAE-CycleGAN models (MI355X-native path)")
    p.add_argument("--runs_dir", type=str, default="runs")
    p.add_argument("--architectures", type=str, nargs="+", default=None)
    p.add_argument("--dataset_filter", type=str, default=None, choices=["hypersim", "summer2winter", "maps", "synthetic"])
    p.add_argument("--num_samples", type=int, default=20)
    p.add_argument("--num_comparison_figures", type=int, default=10)
    p.add_argument("--output_dir", type=str, default="test_results")
    p.add_argument("--no_cuda", action="store_true")
    # additions
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--seed", type=int, default=1234, help="summer2winter y draws and the VAE eps stream")
    p.add_argument("--save_images", action="store_true", help="write every G(x) as a PNG")
    p.add_argument("--ema", action="store_true",
                   help="evaluate the averaged generator weights of runs trained with --ema_decay (a run without them is reported "
                        "and skipped)")
    p.add_argument("--no_swd", action="store_true",
                   help="skip the sliced Wasserstein distance between the translated set and the target set")
    p.add_argument("--reference_split", action="store_true",
                   help="hypersim: evaluate on the reference test.py's random_split(seed 42) subset instead of the run's own")
    return p


# ------------------------------------------------------------------ discovery and grouping (test.py:31-70, 457-468)
def discover_runs(runs_dir="runs"):
    runs = []
    root = Path(runs_dir)
    if not root.exists():
        print(f"Warning: runs directory '{runs_dir}' not found")
        return runs
    for run_dir in sorted(root.iterdir()):
        if not run_dir.is_dir():
            continue
        args_path, best = run_dir / "args.json", run_dir / "best_model.pth"
        if not args_path.exists() or not best.exists():
            print(f"Skipping {run_dir.name}: missing args.json or best_model.pth")
            continue
        with open(args_path) as f:
            args = json.load(f)
        runs.append({"run_dir": run_dir, "run_name": run_dir.name, "architecture": args["architecture"], "args": args,
                     "best_model_path": best})
    return runs


def filter_runs(runs, architectures):
    """--architectures: keep the runs of these architectures (None: all)."""
    return [r for r in runs if r["architecture"] in architectures] if architectures else runs


def get_modality_key(run_args):
    return f"{run_args['source_modality']}_to_{run_args['target_modality']}"


def get_dataset_type(run_args):
    dataset = run_args.get("dataset", "hypersim")
    return "hypersim" if dataset in ("paired", "unpaired") else dataset


# ------------------------------------------------------------------ the generator alone
def translate(model, architecture, x):
    """G(x) of a loaded model — what the reference's test.py takes from model(x[, y])[0] — from the generator alone, in eval mode
    and without autograd: the whole (N, 3, S, S) batch.  double*: decoder_A(encoder(x)), the reconstruction their forward returns
    first.  A VAE generator draws its one eps from the ops stream (the reference samples in eval mode too, Networks.py:225)."""
    arch = train.ALIASES.get(architecture, architecture)
    model.eval()
    with torch.no_grad():
        x = ops.to_nhwc(x)
        if arch == "autoencoder":
            return model(x)
        if arch == "vae":
            return model(x)[0]
        if arch in ("aegan", "cycleae", "cycleaegan"):
            return model.G(x)
        if arch in ("vaegan", "cyclevae", "cyclevaegan"):
            return model.G(x)[0]
        if arch == "doubleae":
            return model.decoder_A(model.encoder(x))
        if arch == "doublevae":
            z, _, _ = model.vae_encoder_block_A(model.encoder(x))
            return model.decoder_A(model.vae_decoder_block_A(z))
    raise ValueError(f"Unknown architecture: {architecture}")


def load_model(run, device, ema=False):
    """test.py:110-143: the model of `run` built from its args.json, with its checkpoint's parameters (`ema`: its averaged
    generator weights, utils.load_model_weights), in eval mode."""
    a = run["args"]
    model = train.create_model(run["architecture"], paired=a.get("paired", True), latent_dim=a.get("latent_dim", 64)).to(device)
    ck = utils.load_model_weights(model, run["best_model_path"], ema=ema)
    model.eval()
    loss = ck.get("loss")
    print(f"  Loaded {run['architecture']} from epoch {ck.get('epoch', 'unknown')}"
          + (f" (loss: {loss:.4f})" if isinstance(loss, float) else ""))
    return model


# ------------------------------------------------------------------ held-out data
class _Head:
    """The first `n` samples of an input_pipeline source."""

    def __init__(self, src, n):
        self.src, self.n = src, min(n, len(src))

    def __len__(self):
        return self.n

    def pair(self, idx, rng):
        return self.src.pair(idx, rng)


def reference_split_indices(n, test_split):
    """The reference test.py's test subset: random_split(..., generator=manual_seed(42)) (:193-196)."""
    ntrain = int((1 - test_split) * n)
    _, test = torch.utils.data.random_split(range(n), [ntrain, n - ntrain], generator=torch.Generator().manual_seed(42))
    return np.asarray(test.indices, dtype=np.int64)


def held_out_indices(n, run_args, reference_split=False):
    """Indices of a hypersim set of n samples that the run held out (train.split_indices, from its --seed and --test_split),
    or the reference test.py's subset; all n when the run held nothing out (test_split 0), as in both."""
    test_split = run_args.get("test_split", 0.1)
    if test_split <= 0:
        return np.arange(n)
    if reference_split:
        return reference_split_indices(n, test_split)
    return train.split_indices(n, test_split, run_args.get("seed", 1234))[1]


def held_out_batches(run_args, architecture, device, num_samples, batch_size, seed, reference_split=False):
    """(count, iterable of {'x', 'y'} device batches): the first `num_samples` held-out samples of a run, `batch_size` at a time,
    through the deterministic Resize((S, S)) + ToTensor recipe."""
    dataset, size = get_dataset_type(run_args), run_args.get("image_size", 256)
    arch = train.ALIASES.get(architecture, architecture)
    if dataset == "synthetic":
        # the held-out stream train.py validates on (seed + 1, epoch 0), drawn at the run's batch size, re-batched
        rb = run_args.get("batch_size", 1)
        loader = train.SyntheticLoader(rb, size, (num_samples + rb - 1) // rb, device, run_args.get("seed", 1234) + 1, 0,
                                       arch in ("autoencoder", "vae"), 0)
        xs, ys = [], []
        for b in loader:
            xs.append(ops.as_phys(b["x"]))
            ys.append(ops.as_phys(b["y"]))
        x, y = ops.logical_of(torch.cat(xs)[:num_samples], 3), ops.logical_of(torch.cat(ys)[:num_samples], 3)
        return len(x), [{"x": x[i:i + batch_size], "y": y[i:i + batch_size]} for i in range(0, len(x), batch_size)]
    root = os.path.join(run_args.get("data_dir", "dataset"), dataset)
    if dataset == "hypersim":
        mods = [run_args["source_modality"], run_args["target_modality"]]
        if mods[0] == mods[1]:
            mods = mods[:1]
        full = input_pipeline.HypersimFolders(root, mods, paired=True)
        src = full.subset(held_out_indices(len(full), run_args, reference_split)[:num_samples])
        same_xy = len(mods) == 1
    else:
        src = _Head(input_pipeline.FolderPairs(root, dataset, "test" if dataset == "summer2winter" else "val"), num_samples)
        same_xy = arch in ("autoencoder", "vae")
    pipe = input_pipeline.DeviceInputPipeline(src, batch_size, size, device, recipe="test", shuffle=False, seed=seed,
                                              num_workers=max(1, run_args.get("num_workers", 1)), same_xy=same_xy)
    return len(src), pipe


# ------------------------------------------------------------------ figures (test.py:345-454), matplotlib loaded on first use
def _plt():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def _figure(rows, col_titles, row_labels, title, path, bold_labels):
    """rows of (input, target, output) HWC images in [0, 1]: one row per entry, titled columns, labelled rows."""
    plt = _plt()
    fig, axes = plt.subplots(len(rows), 3, figsize=(12, 4 * len(rows)))
    axes = np.asarray(axes).reshape(len(rows), 3)
    for r, imgs in enumerate(rows):
        for c, img in enumerate(imgs):
            axes[r, c].imshow(img)
            axes[r, c].set_xticks([])
            axes[r, c].set_yticks([])
            if r == 0:
                axes[r, c].set_title(col_titles[c], fontsize=12)
        axes[r, 0].set_ylabel(row_labels[r], fontsize=10, fontweight="bold" if bold_labels else "normal")
    fig.suptitle(title, fontsize=14, fontweight="bold")
    plt.tight_layout()
    plt.savefig(path, dpi=150, bbox_inches="tight")
    plt.close(fig)


def create_comparison_figure(results, sample_idx, path):
    """One row per model: input, target, G(x) of one sample (test.py:345-391)."""
    _figure([r["images"] for r in results], ["Input (x)", "Target (y)", "Output (G(x))"], [r["model_name"] for r in results],
            f"Sample {sample_idx}", path, bold_labels=True)
    print(f"  Saved comparison figure: {path.name}")


def create_single_model_grid(model_name, samples, path, max_samples=GRID_SAMPLES):
    """One row per sample (at most 8) of one model (test.py:394-444)."""
    n = min(len(samples), max_samples)
    _figure(samples[:n], ["Input", "Target", "Output"], [f"Sample {i + 1}" for i in range(n)], f"Model: {model_name}", path, bold_labels=False)
    print(f"  Saved grid figure: {path.name}")


# ------------------------------------------------------------------ evaluation
def _finite_or_none(v):
    return float(v) if math.isfinite(v) else None


def evaluate_run(model, run, device, args, keep, image_dir=None, paired=True):
    """Translate the run's held-out samples.  Returns (count, host images of the first `keep` samples as (x, y, G(x)) HWC
    float arrays, per-sample metrics (N, 4) float64 or None, images/s, the sliced Wasserstein entry or None).  The distance is
    fed (G(x), y) of every batch; its time is not part of images/s."""
    count, batches = held_out_batches(run["args"], run["architecture"], device, args.num_samples, args.batch_size, args.seed,
                                      args.reference_split)
    dist, dist_time = None, 0.0
    if not getattr(args, "no_swd", False):
        try:
            dist = swd.SlicedWasserstein(run["args"].get("image_size", 256), count, args.seed)
        except RuntimeError as e:                    # a size the metric refuses: reported, not fatal
            print(f"  {run['run_name']}: no SWD: {e}")
    ops.manual_seed(args.seed)                       # the eps of every run starts at the same place, whatever ran before
    kept, metrics, done = [], [], 0
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for batch in batches:
        x, y = batch["x"], batch["y"]
        gx = translate(model, run["architecture"], x)
        if paired:
            metrics.append(ops.image_metrics(gx, y))
        if dist is not None:
            torch.cuda.synchronize(device)
            s0 = time.perf_counter()
            dist.add(gx, y)
            torch.cuda.synchronize(device)
            dist_time += time.perf_counter() - s0
        nb = x.shape[0]
        take = max(0, min(nb, keep - done))
        if take:
            shown = [ops.to_display(t[:take]).cpu().numpy() for t in (x, y, gx)]
            kept.extend(zip(*shown))
        if image_dir is not None:
            from PIL import Image
            u8 = ops.to_display(gx, uint8=True).cpu().numpy()
            for i in range(nb):
                Image.fromarray(u8[i]).save(image_dir / f"sample_{done + i:04d}.png")
        done += nb
    per_sample = torch.cat(metrics).cpu().double().numpy() if metrics else None
    torch.cuda.synchronize(device)
    ips = done / max(time.perf_counter() - t0 - dist_time, 1e-9)
    return count, kept, per_sample, ips, dist.result() if dist is not None else None


def _metrics_entry(per_sample):
    if per_sample is None:
        return None, None
    means = {k: _finite_or_none(float(per_sample[:, i].mean())) for i, k in enumerate(METRIC_NAMES)}
    means["num_samples"] = int(per_sample.shape[0])
    lists = {k: [_finite_or_none(float(v)) for v in per_sample[:, i]] for i, k in enumerate(METRIC_NAMES)}
    return means, lists


def evaluate_model_group(runs, device, output_dir, args, unpaired=False):
    """test.py:470-604, one model at a time: per modality group, the comparison figures, a grid per model and summary.json."""
    output_dir.mkdir(parents=True, exist_ok=True)
    groups = {}
    for run in runs:
        groups.setdefault(get_modality_key(run["args"]), []).append(run)
    print(f"\nFound {len(groups)} modality configuration(s):")
    for key, group in groups.items():
        print(f"  - {key}: {len(group)} model(s)")
    keep = max(args.num_comparison_figures, GRID_SAMPLES)
    for key, group in groups.items():
        print(f"\n{'-' * 60}\nProcessing modality: {key}\n{'-' * 60}")
        gdir = output_dir / key
        gdir.mkdir(parents=True, exist_ok=True)
        done = []
        for run in group:
            try:
                model = load_model(run, device, ema=getattr(args, "ema", False))
            except Exception as e:                       # as the reference: a run that does not load is reported and skipped
                print(f"Error loading {run['run_name']}: {e}")
                continue
            image_dir = None
            if args.save_images:
                image_dir = gdir / "images" / run["run_name"]
                image_dir.mkdir(parents=True, exist_ok=True)
            count, kept, per_sample, ips, dist = evaluate_run(model, run, device, args, keep, image_dir, paired=not unpaired)
            print(f"  {run['run_name']}: {count} samples, {ips:.1f} images/s")
            if dist is not None:
                print(f"  {run['run_name']}: SWD x1e3 " + " ".join(f"{k}: {'n/a' if v is None else format(v, '.2f')}"
                                                                  for k, v in list(dist["levels"].items()) + [("mean", dist["mean"])]))
            done.append({"run": run, "count": count, "kept": kept, "per_sample": per_sample, "swd": dist})
            del model
        if not done:
            print("No models loaded successfully for this group!")
            continue
        nfig = min(args.num_comparison_figures, min(len(d["kept"]) for d in done))
        for i in range(nfig):
            create_comparison_figure([{"model_name": d["run"]["run_name"], "images": d["kept"][i]} for d in done], i,
                                     gdir / f"comparison_sample_{i:04d}.png")
        print("\nGenerating per-model grids...")
        for d in done:
            if d["kept"]:
                create_single_model_grid(d["run"]["run_name"], d["kept"], gdir / f"grid_{d['run']['run_name']}.png")
        ref = done[0]["run"]["args"]
        models = []
        for d in done:
            means, lists = _metrics_entry(d["per_sample"])
            models.append({"name": d["run"]["run_name"], "architecture": d["run"]["architecture"],
                           "checkpoint": str(d["run"]["best_model_path"]), "training_args": d["run"]["args"],
                           "metrics": means, "per_sample": lists})
            if not getattr(args, "no_swd", False):
                models[-1]["swd"] = d["swd"]
        summary = {"modality": key, "source_modality": ref["source_modality"], "target_modality": ref["target_modality"],
                   "num_models": len(done), "num_samples": done[0]["count"], "unpaired": unpaired, "models": models}
        with open(gdir / "summary.json", "w") as f:
            json.dump(summary, f, indent=2, allow_nan=False)
        print(f"\nSaved summary to: {gdir / 'summary.json'}")


DATASETS = ("hypersim", "summer2winter", "maps", "synthetic")


def main(args):
    """test.py:607-690.  Returns the output directory."""
    if args.no_cuda or not torch.cuda.is_available():
        raise RuntimeError("this path has no CPU implementation: an MI355X is required (the reference's own "
                           "test.py is the CPU path)")
    if args.batch_size < 1 or args.num_samples < 1:
        raise ValueError("--batch_size and --num_samples must be at least 1")
    device = torch.device("cuda", torch.cuda.current_device())
    print(f"Using device: {device}")
    output_dir = Path(args.output_dir) / f"test_results_{datetime.now().strftime('%Y%m%d_%H%M%S')}"
    output_dir.mkdir(parents=True, exist_ok=True)
    print(f"Output directory: {output_dir}")
    runs = discover_runs(args.runs_dir)
    if not runs:
        print("No trained models found!")
        return output_dir
    print(f"\nDiscovered {len(runs)} trained models:")
    for run in runs:
        print(f"  - {run['run_name']} ({run['architecture']})")
    if args.architectures:
        runs = filter_runs(runs, args.architectures)
        print(f"\nFiltered to {len(runs)} models matching architectures: {args.architectures}")
    for dataset in DATASETS:
        group = [r for r in runs if get_dataset_type(r["args"]) == dataset]
        if group and args.dataset_filter in (None, dataset):
            print(f"\n{'=' * 60}\nEvaluating {len(group)} {dataset} dataset models\n{'=' * 60}")
            evaluate_model_group(group, device, output_dir / dataset, args, unpaired=dataset == "summer2winter")
    print(f"\n{'=' * 60}\nEvaluation complete!\nResults saved to: {output_dir}\n{'=' * 60}")
    return output_dir


if __name__ == "__main__":
    main(build_parser().parse_args())
