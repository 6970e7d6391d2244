"""GPU: the sampling translator end to end — translate.sample_images (one encoder pass, K decodes in chunks, the statistics the
kernels of csrc/sample_stats.hip accumulate) against the one-draw path it generalises, and `translate.py --samples K`.

The models carry synthetic parameters (pkg.synth), as in tests/test_gpu_translate.py, with latent 64."""
import argparse
import ctypes
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED_P = 20261016
OUT_BOUND = 1e-3                      # the parity suite's bound on generator outputs: max-abs error over the output's largest magnitude
ARCH_DIRS = [("vae", "a2b"), ("cyclevaegan", "a2b"), ("cyclevaegan", "b2a"), ("doublevae", "a2b"), ("doublevae", "b2a")]


def acc_bound(k):
    """tests/test_gpu_sample_stats.py: at most eight fp32 roundings of quantities <= 1 per Welford update, k updates."""
    return k * 2.0 ** -21


@pytest.fixture(scope="module")
def tr(pkg):
    return importlib.import_module("vae-cyclegan-implementation_amd.translate")


def _synth_into(pkg, module, prefix):
    shapes = {prefix + k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = pkg.synth.state_dict_like(shapes, SEED_P, bias_std=0.02)
    module.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items()})
    pkg.ops.PARAM_EPOCH[0] += 1


@pytest.fixture(scope="module")
def models(pkg):
    N = pkg.Networks
    cache = {}

    def get(arch):
        if arch not in cache:
            torch.manual_seed(5)
            if arch == "autoencoder":
                m = N.Autoencoder()
                _synth_into(pkg, m, "ae.")
            elif arch == "vae":
                m = N.VariationalAutoencoder(latent_dim=64)
                _synth_into(pkg, m, "vae.")
            elif arch == "cyclevaegan":
                m = N.CycleVAEGAN(latent_dim=64, paired=False)
                _synth_into(pkg, m.G, "cvg.G.")
                _synth_into(pkg, m.F, "cvg.F.")
            elif arch == "doublevae":
                m = N.DoubleVariationalAutoencoder(latent_dim=64)
                _synth_into(pkg, m, "dvae.")
            cache[arch] = m.to(DEV).eval()
        return cache[arch]
    return get


def _frames(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3), dtype=np.uint8)


def _stats64(samples):
    """float64 mean (N, H, W, 3) and spread (N, H, W) of fp32 samples (N, K, H, W, 3)."""
    x = samples.double().cpu().numpy()
    return x.mean(axis=1), np.sqrt(x.var(axis=1, ddof=1).sum(axis=3) / 3.0)


def _spread_tolerance(s64, k):
    """m2 / (K - 1) is within B = acc_bound(K) per channel, so is their mean v; s = sqrt(v): |ds| <= sqrt(B) always, and
    |ds| = |dv| / (s + s') <= B / s where s > 2 sqrt(B) (then s' >= s / 2); plus the spread kernel's 2 ulp."""
    b = acc_bound(k)
    return np.where(s64 > 2 * math.sqrt(b), b / np.maximum(s64, 1e-30), math.sqrt(b)) + 2 * np.spacing(s64.astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------ one encode
def test_one_encoder_pass_and_one_decode_per_chunk(pkg, tr, models, monkeypatch):
    model = models("vae")
    calls = {"encode": 0, "decode": 0, "batches": []}
    enc, dec = model.encoder.forward, model.decoder.forward

    def counted_enc(x):
        calls["encode"] += 1
        return enc(x)

    def counted_dec(x):
        calls["decode"] += 1
        calls["batches"].append(x.shape[0])
        return dec(x)
    monkeypatch.setattr(model.encoder, "forward", counted_enc)
    monkeypatch.setattr(model.decoder, "forward", counted_dec)
    res = tr.sample_images(model, "vae", _frames(1, 32, 48, 1), 4, chunk=2)
    assert calls == {"encode": 1, "decode": 2, "batches": [2, 2]}
    assert res["samples"].dtype == torch.uint8 and tuple(res["samples"].shape) == (1, 4, 32, 48, 3)
    assert res["mean"].dtype == torch.uint8 and tuple(res["mean"].shape) == (1, 32, 48, 3)
    assert res["spread"].dtype == torch.float32 and tuple(res["spread"].shape) == (1, 32, 48)
    assert res["spread_u8"].dtype == torch.uint8 and tuple(res["spread_u8"].shape) == (1, 32, 48)
    assert tuple(res["mean_spread"].shape) == (1,) and all(v.device.type == "cuda" for v in res.values())
    calls.update(encode=0, decode=0, batches=[])
    tr.sample_images(model, "vae", _frames(2, 32, 48, 1), 3)
    assert calls == {"encode": 1, "decode": 1, "batches": [6]}


# ------------------------------------------------------------------ each sample is a translation
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("h,w", [(32, 48), (96, 160)])
@pytest.mark.parametrize("arch,direction", ARCH_DIRS)
def test_each_sample_is_the_translation_with_its_eps(pkg, tr, models, arch, direction, h, w, n):
    ops = pkg.ops
    K = 3
    model = models(arch)
    u8 = _frames(n, h, w, h + w + n)
    eps = torch.from_numpy(pkg.synth.normal((n, K, 64, h // 16, w // 16), SEED_P, f"eps/{arch}/{direction}/{n}x{h}x{w}"))
    res = tr.sample_images(model, arch, u8, K, direction=direction, eps=eps, debug=True)
    got = res["samples"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, K, h, w, 3) and bool(torch.isfinite(got).all())
    assert torch.equal(res["eps"].contiguous().cpu(), eps)
    worst = 0.0
    for i in range(n):
        x, window = ops.image_load(torch.from_numpy(u8[i:i + 1]).to(DEV))
        for j in range(K):
            ops.inject_eps([eps[i, j][None]])
            y = tr.run_generator(model, arch, x, direction, "sample", None)
            want = ops.to_display_hw(y, window)[0]
            err = float((got[i, j] - want).abs().max() / y.abs().max())
            worst = max(worst, err)
            assert err <= OUT_BOUND, f"sample ({i}, {j}): max-abs error {err:.3e} of the output's amax"
    inside = float(((got > 0) & (got < 1)).float().mean())
    print(f"{arch} {direction} {n}x{h}x{w}: worst max-abs/amax {worst:.3e}; {inside:.1%} of the sample values inside (0, 1)")
    assert inside > 0 and not torch.equal(got[:, 0], got[:, 1])           # the comparison saw values the clamp left alone
    assert not ops._EPS_QUEUE


# ------------------------------------------------------------------ the statistics are those of the samples
@pytest.mark.parametrize("arch,direction,n,h,w,chunk", [("vae", "a2b", 2, 40, 56, 2), ("cyclevaegan", "b2a", 1, 96, 160, None)])
def test_mean_and_spread_are_those_of_the_returned_samples(pkg, tr, models, arch, direction, n, h, w, chunk):
    K = 5
    model = models(arch)
    u8 = _frames(n, h, w, 7)
    res = tr.sample_images(model, arch, u8, K, direction=direction, seed=3, chunk=chunk, debug=True)
    mean64, s64 = _stats64(res["samples"])
    e_mean = float(np.abs(res["mean"].cpu().numpy() - mean64).max())
    err_s = np.abs(res["spread"].cpu().numpy().astype(np.float64) - s64)
    tol = _spread_tolerance(s64, K)
    print(f"{arch} {n}x{h}x{w}: max |mean - fp64| {e_mean:.3e} (bound {acc_bound(K):.3e}); max spread error / tolerance "
          f"{float((err_s / tol).max()):.3e}; spread max {s64.max():.4f} mean {s64.mean():.5f}")
    assert e_mean <= acc_bound(K)
    assert (err_s <= tol).all()
    assert s64.max() > 0, "the samples of a variational generator differ"
    ms = res["mean_spread"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(ms - s64.mean(axis=(1, 2))) <= tol.mean(axis=(1, 2)) + 1e-6 * s64.mean(axis=(1, 2)))
    # the uint8 forms are the display conversions of the same numbers
    plain = tr.sample_images(model, arch, u8, K, direction=direction, seed=3, chunk=chunk)
    to_u8 = lambda t: np.clip(np.floor(255.0 * t.cpu().numpy().astype(np.float64) + 0.5), 0, 255).astype(np.uint8)
    assert np.array_equal(plain["samples"].cpu().numpy(), to_u8(res["samples"]))
    assert np.array_equal(plain["mean"].cpu().numpy(), to_u8(res["mean"]))
    assert torch.equal(plain["spread"].view(torch.int32), res["spread"].view(torch.int32))
    v = 255.0 * np.minimum(1.0, 2.0 * res["spread"].cpu().numpy().astype(np.float64)) + 0.5
    far = np.abs(v - np.rint(v)) > 1e-4                                    # spread_u8 is made from the unrounded s: skip the ties of its fp32 form
    assert np.array_equal(plain["spread_u8"].cpu().numpy()[far], np.floor(v).astype(np.uint8)[far])


# ------------------------------------------------------------------ the eps stream
def test_seed_chunking_and_stream_position(pkg, tr, models):
    ops = pkg.ops
    model = models("vae")
    n, K, h, w = 2, 4, 32, 48
    u8 = _frames(n, h, w, 9)
    a = tr.sample_images(model, "vae", u8, K, seed=21, debug=True)
    per = 64 * (h // 16) * (w // 16)
    assert ops._RNG["offset"] == n * K * per // 4 and ops._RNG["seed"] == 21
    b = tr.sample_images(model, "vae", u8, K, seed=21, debug=True)
    for key in ("samples", "mean", "spread", "spread_u8", "mean_spread", "eps"):
        assert torch.equal(a[key].contiguous().view(torch.uint8), b[key].contiguous().view(torch.uint8)), key
    c = tr.sample_images(model, "vae", u8, K, seed=22, debug=True)
    assert not torch.equal(a["eps"], c["eps"]) and not torch.equal(a["samples"], c["samples"])
    ones = tr.sample_images(model, "vae", u8, K, seed=21, chunk=1, debug=True)
    assert ops._RNG["offset"] == n * K * per // 4, "the stream advances once per batch, not per chunk"
    assert torch.equal(ones["eps"].contiguous().view(torch.int32), a["eps"].contiguous().view(torch.int32))
    assert float((ones["samples"] - a["samples"]).abs().max()) <= OUT_BOUND * float(a["samples"].abs().max())
    # the draws are vcg_randn's at the documented positions, sample (n, j) at (n K + j) per / 4
    want = torch.stack([ops.randn((h // 16, w // 16, 64), DEV, 21, i * per // 4) for i in range(n * K)])
    got = a["eps"].reshape(n * K, 64, h // 16, w // 16).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # seed None: the stream goes on where it is
    ops.manual_seed(21)
    ops._RNG["offset"] = 1000
    tr.sample_images(model, "vae", u8, K, seed=None)
    assert ops._RNG["offset"] == 1000 + n * K * per // 4


# ------------------------------------------------------------------ temperature
def test_temperature_zero_decodes_the_mean_k_times(pkg, tr, models):
    model = models("cyclevaegan")
    u8 = _frames(2, 48, 64, 13)
    res = tr.sample_images(model, "cyclevaegan", u8, 3, direction="b2a", temperature=0.0, debug=True)
    mean_out = tr.translate_images(model, "cyclevaegan", u8, direction="b2a", eps="mean", return_float=True)
    amax = float(mean_out.abs().max())
    for j in range(3):
        assert float((res["samples"][:, j] - mean_out).abs().max()) <= OUT_BOUND * amax, j
    same = (res["samples"] == res["samples"][:, :1]).all(dim=1).all(dim=-1)           # (N, H, W): the K samples agree bitwise
    assert bool(same.any())
    assert bool((res["spread"][same] == 0).all()) and bool((res["spread_u8"][same] == 0).all())


# ------------------------------------------------------------------ refusals on the device path
def test_refusals_with_models_on_the_device(pkg, tr, models):
    ops, lib = pkg.ops, pkg._native.lib()
    with pytest.raises(ValueError, match="not variational"):
        tr.sample_images(models("autoencoder"), "autoencoder", _frames(1, 32, 48, 1), 4)
    model = models("vae")
    n = ops.MAX_TRANSLATE_PIXELS // (768 * 1024) + 1
    frames = torch.zeros((n, 768, 1024, 3), dtype=torch.uint8)             # on the host
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    lib.vcg_profile_enable(1)
    try:
        with pytest.raises(RuntimeError, match=f"MAX_TRANSLATE_PIXELS = {ops.MAX_TRANSLATE_PIXELS}"):
            tr.sample_images(model, "vae", frames, 2)
        need = lib.vcg_profile_read(None, 0)
        buf = ctypes.create_string_buffer(max(int(need), 0) + 16)
        lib.vcg_profile_read(buf, len(buf))
    finally:
        lib.vcg_profile_enable(0)
    assert not buf.value.strip(), f"convolution kernels were launched: {buf.value[:200]}"
    assert torch.cuda.memory_allocated(DEV) == before
    with pytest.raises(RuntimeError, match="eps has shape"):
        tr.sample_images(model, "vae", _frames(1, 32, 48, 1), 4, eps=torch.zeros(1, 3, 64, 2, 3))


# ------------------------------------------------------------------ the command line
def test_cli_end_to_end(pkg, tr, tmp_path):
    from PIL import Image
    utils = pkg.utils
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")
    rng = np.random.RandomState(48)
    src, tgt = tmp_path / "in", tmp_path / "targets"
    src.mkdir()
    tgt.mkdir()
    for name in ("a.png", "b.png"):
        Image.fromarray(rng.randint(0, 256, (40, 56, 3), dtype=np.uint8)).save(src / name)
        Image.fromarray(rng.randint(0, 256, (40, 56, 3), dtype=np.uint8)).save(tgt / name)
    run = tmp_path / "run"
    run.mkdir()
    torch.manual_seed(31)
    model = train.create_model("vae", paired=False, latent_dim=64).to(DEV).eval()
    args = argparse.Namespace(architecture="vae", latent_dim=64, paired=False, image_size=256)
    model.configure_optimizers(lr=2e-4)
    utils.save_checkpoint(model, 3, 0.25, args, str(run / "best_model.pth"))
    with open(run / "args.json", "w") as f:
        json.dump(vars(args), f)
    base = ["--checkpoint", str(run), "--input", str(src), "--batch_size", "2", "--seed", "17"]
    out = tmp_path / "out"
    assert tr.main(base + ["--output", str(out), "--samples", "3", "--targets", str(tgt)]) == 0
    want_files = [f"{s}_translated_{t}.png" for s in "ab" for t in ("s00", "s01", "s02", "mean", "spread")] + ["metrics.json"]
    assert sorted(os.listdir(out)) == sorted(want_files)
    loaded, arch = tr.load_generator(run, device=DEV)
    frames = [np.asarray(Image.open(src / n)) for n in ("a.png", "b.png")]
    res = tr.sample_images(loaded, arch, frames, 3, seed=17)
    for i, s in enumerate("ab"):
        for j in range(3):
            assert np.array_equal(np.asarray(Image.open(out / f"{s}_translated_s{j:02d}.png")), res["samples"][i, j].cpu().numpy()), (s, j)
        assert np.array_equal(np.asarray(Image.open(out / f"{s}_translated_mean.png")), res["mean"][i].cpu().numpy())
        spread = Image.open(out / f"{s}_translated_spread.png")
        assert spread.mode == "L" and np.array_equal(np.asarray(spread), res["spread_u8"][i].cpu().numpy())
    rep = json.load(open(out / "metrics.json"))
    assert rep["num_files"] == 2 and set(rep["mean"]) == set(tr.METRIC_NAMES)
    for i, name in enumerate(("a.png", "b.png")):
        entry = rep["per_file"][name]
        assert len(entry["samples"]) == 3 and all(set(m) == set(tr.METRIC_NAMES) for m in entry["samples"])
        assert math.isfinite(entry["mean_spread"]) and entry["mean_spread"] == float(res["mean_spread"][i].cpu().double())
        assert all(math.isfinite(entry[k]) for k in tr.METRIC_NAMES)
        assert entry["samples"][0]["l1"] != entry["samples"][1]["l1"]
    # without --targets: samples.json; with --size: the evaluator's square resize
    out_s = tmp_path / "out_size"
    assert tr.main(base + ["--output", str(out_s), "--samples", "2", "--size", "64", "--spread_gain", "8"]) == 0
    assert sorted(os.listdir(out_s)) == sorted([f"{s}_translated_{t}.png" for s in "ab" for t in ("s00", "s01", "mean", "spread")]
                                               + ["samples.json"])
    assert Image.open(out_s / "a_translated_s01.png").size == (64, 64) and Image.open(out_s / "b_translated_spread.png").size == (64, 64)
    rep = json.load(open(out_s / "samples.json"))
    assert rep["num_files"] == 2 and all(math.isfinite(v["mean_spread"]) for v in rep["per_file"].values())
    # without --samples: the bytes of the one-draw path, untouched
    out1 = tmp_path / "out1"
    assert tr.main(base + ["--output", str(out1)]) == 0
    assert sorted(os.listdir(out1)) == ["a_translated.png", "b_translated.png"]
    want = tr.translate_images(loaded, arch, frames, seed=17).cpu().numpy()
    for i, s in enumerate("ab"):
        assert np.array_equal(np.asarray(Image.open(out1 / f"{s}_translated.png")), want[i]), s
