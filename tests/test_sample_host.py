"""CPU: the host side of the sampling translator (translate.py --samples K) — the parser, every refusal before a device is
touched, the chunk planner, the output names, the report files with the device call stubbed out, and the argument checks of the
four new C entry points (csrc/sample_stats.hip) without a GPU."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vcg_reparam_many_fwd", "vcg_sample_accumulate", "vcg_spread_workspace", "vcg_spread_display_hw")
BASE = ["--checkpoint", "run", "--input", "in", "--output", "out"]


@pytest.fixture(scope="module")
def tr(pkg):
    return importlib.import_module("vae-cyclegan-implementation_amd.translate")


class Halves:
    """A model as far as sampler_of looks at it."""
    latent, decode = "latent", "decode"


class Cycle:
    G, F = Halves(), Halves()


# ------------------------------------------------------------------ parser
def test_parser_takes_the_three_flags(tr):
    a = tr.build_parser().parse_args(BASE)
    assert (a.samples, a.temperature, a.spread_gain) == (1, 1.0, 2.0)
    a = tr.build_parser().parse_args(BASE + ["--samples", "8", "--temperature", "0.5", "--spread_gain", "6"])
    assert (a.samples, a.temperature, a.spread_gain) == (8, 0.5, 6.0)
    text = tr.build_parser().format_help()
    assert "derived, not tuned" in " ".join(text.split()) and "usually raise it" in " ".join(text.split())
    spec = importlib.util.spec_from_file_location("_translate_shim2", os.path.join(ROOT, "translate.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    assert shim.sample_images is tr.sample_images


# ------------------------------------------------------------------ refusals before a device is touched
def test_cli_refusals_come_before_the_device_and_any_file(tr, tmp_path, monkeypatch):
    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(tr, "_device", no_device)
    monkeypatch.setattr(tr, "discover_inputs", lambda p: (_ for _ in ()).throw(AssertionError("the input was read")))
    vae = ["--architecture", "vae"]
    with pytest.raises(ValueError, match="--eps mean"):
        tr.main(BASE + vae + ["--samples", "4", "--eps", "mean"])
    with pytest.raises(ValueError, match="--samples of at least 2"):
        tr.main(BASE + vae + ["--temperature", "0.7"])
    with pytest.raises(ValueError, match="--samples of at least 2"):
        tr.main(BASE + vae + ["--temperature", "0.7", "--samples", "1"])
    for arch in ("autoencoder", "aegan", "cycleae", "cycleaegan", "doubleae"):
        with pytest.raises(ValueError, match="variational checkpoint"):
            tr.main(BASE + ["--architecture", arch, "--samples", "2"])
    run = tmp_path / "run"                                                  # a run directory says what it is in args.json
    run.mkdir()
    (run / "args.json").write_text(json.dumps({"architecture": "cycleaegan"}))
    with pytest.raises(ValueError, match="variational checkpoint.*cycleaegan"):
        tr.main(["--checkpoint", str(run), "--input", "in", "--output", "out", "--samples", "3"])
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(ValueError, match="temperature"):
            tr.main(BASE + vae + ["--samples", "2", "--temperature", bad])
    with pytest.raises(ValueError, match="--spread_gain"):
        tr.main(BASE + vae + ["--samples", "2", "--spread_gain", "-2"])
    with pytest.raises(ValueError, match="--samples must be at least 1"):
        tr.main(BASE + vae + ["--samples", "0"])
    # what passes these checks goes on to the device
    with pytest.raises(AssertionError, match="device was asked"):
        tr.main(BASE + vae + ["--samples", "2", "--temperature", "0"])
    (run / "args.json").write_text(json.dumps({"architecture": "cyclevaegan"}))
    with pytest.raises(AssertionError, match="device was asked"):
        tr.main(["--checkpoint", str(run), "--input", "in", "--output", "out", "--samples", "3"])


def test_sample_images_refuses_before_the_device(tr):
    """Frames on the host, models that are no modules: whatever is refused here has touched neither."""
    frames = np.zeros((1, 64, 64, 3), np.uint8)
    for arch in ("autoencoder", "aegan", "cycleae", "cycleaegan", "doubleae"):
        with pytest.raises(ValueError, match="not variational"):
            tr.sample_images(object(), arch, frames, 4)
    with pytest.raises(ValueError, match="Unknown"):
        tr.sample_images(object(), "pix2pix", frames, 4)
    for k in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2"):
            tr.sample_images(Halves(), "vae", frames, k)
    with pytest.raises(ValueError, match="one generator"):
        tr.sample_images(Halves(), "vae", frames, 4, direction="b2a")
    with pytest.raises(ValueError, match="direction"):
        tr.sample_images(Cycle(), "cyclevaegan", frames, 4, direction="sideways")
    with pytest.raises(ValueError, match="temperature"):
        tr.sample_images(Halves(), "vae", frames, 4, temperature=-0.5)
    with pytest.raises(RuntimeError, match="smaller than 32"):
        tr.sample_images(Halves(), "vae", np.zeros((1, 16, 64, 3), np.uint8), 4)
    with pytest.raises(RuntimeError, match="MAX_TRANSLATE_PIXELS"):
        tr.sample_images(Halves(), "vae", torch.zeros((11, 768, 1024, 1), dtype=torch.uint8), 2)
    assert tr.sampler_of(Cycle(), "cyclevae", "b2a") == ("latent", "decode")
    assert tr.sampler_of(Halves(), "vae") == ("latent", "decode")


def test_double_vae_sides(pkg):
    """translate_A_to_B samples block B and decodes with decoder_B; the methods name that side, and refuse any other."""
    m = pkg.Networks.DoubleVariationalAutoencoder.__new__(pkg.Networks.DoubleVariationalAutoencoder)
    with pytest.raises(ValueError, match="'A' or 'B'"):
        m.decode(None, "C")
    with pytest.raises(ValueError, match="'A' or 'B'"):
        m.latent(None, "a2b")


# ------------------------------------------------------------------ the chunk plan
@pytest.mark.parametrize("n,hp,wp,samples,chunk", [(1, 768, 1024, 16, None), (1, 768, 1024, 10, None), (1, 768, 1024, 11, None),
                                                   (2, 768, 1024, 16, None), (1, 32, 48, 7, None), (1, 32, 48, 7, 3), (3, 96, 160, 5, 1),
                                                   (1, 768, 1024, 16, 4), (1, 768, 1024, 16, 64), (10, 768, 1024, 3, None)])
def test_sample_chunks_cover_every_sample_once_in_order(tr, pkg, n, hp, wp, samples, chunk):
    plan = tr.sample_chunks(n, hp, wp, samples, chunk)
    assert [j for first, k in plan for j in range(first, first + k)] == list(range(samples))
    assert all(k >= 1 and n * k * hp * wp <= pkg.ops.MAX_TRANSLATE_PIXELS for _, k in plan)
    if chunk is not None:
        assert all(k <= chunk for _, k in plan)
    largest = min(samples, pkg.ops.MAX_TRANSLATE_PIXELS // (n * hp * wp), chunk or samples)
    assert all(k == largest for _, k in plan[:-1]) and plan[-1][1] <= largest       # as few decodes as the bound allows


def test_sample_chunks_at_the_frame_the_bound_was_set_for(tr):
    assert tr.sample_chunks(1, 768, 1024, 16) == [(0, 10), (10, 6)]
    assert max(k for _, k in tr.sample_chunks(1, 768, 1024, 16)) <= 10
    assert tr.sample_chunks(1, 768, 1024, 16, chunk=4) == [(0, 4), (4, 4), (8, 4), (12, 4)]
    assert tr.sample_chunks(2, 48, 64, 5, chunk=2) == [(0, 2), (2, 2), (4, 1)]
    assert tr.sample_chunks(1, 48, 64, 3) == [(0, 3)]
    with pytest.raises(ValueError):
        tr.sample_chunks(1, 48, 64, 3, chunk=0)
    with pytest.raises(ValueError):
        tr.sample_chunks(11, 768, 1024, 3)


# ------------------------------------------------------------------ files
def test_output_names(tr):
    names = tr.sample_output_names("x/y/frame.0001.jpg", 3, "_B")
    assert names == {"samples": ["frame.0001_B_s00.png", "frame.0001_B_s01.png", "frame.0001_B_s02.png"], "mean": "frame.0001_B_mean.png",
                     "spread": "frame.0001_B_spread.png"}
    many = tr.sample_output_names("a.png", 101)["samples"]
    assert many[0] == "a_translated_s00.png" and many[9] == "a_translated_s09.png" and many[100] == "a_translated_s100.png"
    assert len(set(many)) == 101


def _write_images(folder, specs):
    from PIL import Image
    rng = np.random.RandomState(3)
    folder.mkdir(parents=True, exist_ok=True)
    for name, shape in specs:
        Image.fromarray(rng.randint(0, 256, shape, dtype=np.uint8)).save(folder / name)


def test_main_writes_samples_mean_spread_and_reports(tr, tmp_path, monkeypatch):
    """The CLI's file handling with the device call stubbed out: names, grey spread PNGs, samples.json / metrics.json."""
    from PIL import Image
    _write_images(tmp_path / "in", [("a.png", (40, 56, 3)), ("b.png", (40, 56, 3))])
    _write_images(tmp_path / "tg", [("a.png", (40, 56, 3)), ("b.png", (40, 56, 3))])
    calls = []

    def fake(model, architecture, frames, targets, args, device):
        n, h, w, _ = frames.shape
        k = args.samples
        calls.append((n, k, args.temperature, args.spread_gain, targets is not None))
        res = dict(samples=torch.stack([frames[..., :3] // (j + 1) for j in range(k)], dim=1), mean=frames[..., :3].clone(),
                   spread_u8=torch.full((n, h, w), 7, dtype=torch.uint8), mean_spread=torch.tensor([0.25, 0.5][:n]))
        if targets is not None:
            res["metrics"] = torch.tensor([[0.5, 0.0, float("inf"), 1.0]] * n)
            res["sample_metrics"] = torch.arange(n * k * 4, dtype=torch.float32).view(n, k, 4)
        return res

    monkeypatch.setattr(tr, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(tr, "load_generator", lambda *a, **k: (Halves(), "vae"))
    monkeypatch.setattr(tr, "run_batch_sampled", fake)
    monkeypatch.setattr(tr, "run_batch", lambda *a: (_ for _ in ()).throw(AssertionError("the one-draw path ran")))
    argv = ["--checkpoint", "m.pth", "--architecture", "vae", "--input", str(tmp_path / "in"), "--batch_size", "2", "--samples", "3",
            "--temperature", "0.5", "--spread_gain", "4"]
    assert tr.main(argv + ["--output", str(tmp_path / "out")]) == 0
    assert calls == [(2, 3, 0.5, 4.0, False)]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(
        [f"{s}_translated_{t}.png" for s in "ab" for t in ("s00", "s01", "s02", "mean", "spread")] + ["samples.json"])
    a = tr.decode(tmp_path / "in" / "a.png")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "a_translated_s01.png")), a // 2)
    spread = Image.open(tmp_path / "out" / "b_translated_spread.png")
    assert spread.mode == "L" and np.array_equal(np.asarray(spread), np.full((40, 56), 7, np.uint8))
    assert json.load(open(tmp_path / "out" / "samples.json")) == {"num_files": 2, "per_file": {"a.png": {"mean_spread": 0.25},
                                                                                                 "b.png": {"mean_spread": 0.5}}}
    assert tr.main(argv + ["--output", str(tmp_path / "out2"), "--targets", str(tmp_path / "tg")]) == 0
    rep = json.load(open(tmp_path / "out2" / "metrics.json"))
    assert not (tmp_path / "out2" / "samples.json").exists()
    assert rep["num_files"] == 2 and rep["mean"] == {"l1": 0.5, "mse": 0.0, "psnr": None, "ssim": 1.0}
    b = rep["per_file"]["b.png"]
    assert {k: b[k] for k in tr.METRIC_NAMES} == {"l1": 0.5, "mse": 0.0, "psnr": None, "ssim": 1.0} and b["mean_spread"] == 0.5
    assert b["samples"] == [dict(zip(tr.METRIC_NAMES, (float(v) for v in range(12 + 4 * j, 16 + 4 * j)))) for j in range(3)]


# ------------------------------------------------------------------ C ABI
def test_new_entry_points_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "vcg.h")).read()
    lib = ctypes.CDLL(pkg._native.build())
    for s in NEW_SYMBOLS:
        assert s + "(" in header and hasattr(lib, s) and s in pkg._native.SIGNATURES, s
    assert "sample_stats.hip" in pkg._native.SOURCES
    assert header.count("new: the reference has no inference path") >= 3
    assert pkg._native.lib().vcg_abi_version() == 6


def test_new_entry_points_reject_bad_arguments_without_touching_the_gpu(pkg):
    lib = pkg._native.lib()
    err = lambda: lib.vcg_last_error()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)                  # never dereferenced: every call below fails its checks
    nan, inf = float("nan"), float("inf")
    rp = lib.vcg_reparam_many_fwd
    assert rp(None, p, None, None, p, 1, 1, 0, 1, 4, 1.0, 0, 0, None) != 0 and b"null" in err()
    assert rp(p, p, None, None, None, 1, 1, 0, 1, 4, 1.0, 0, 0, None) != 0 and b"null" in err()
    for n, K, k in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-2, 4, 1), (1, 4, -1)):
        assert rp(p, p, None, None, p, n, K, 0, k, 4, 1.0, 0, 0, None) != 0 and b"at least 1" in err()
    assert rp(p, p, None, None, p, 1, 5, 3, 3, 4, 1.0, 0, 0, None) != 0 and b"leave" in err()
    assert rp(p, p, None, None, p, 1, 5, -1, 2, 4, 1.0, 0, 0, None) != 0 and b"leave" in err()
    assert rp(p, p, None, None, p, 1, 5, 2 ** 31 - 1, 2, 4, 1.0, 0, 0, None) != 0 and b"leave" in err()
    for per in (0, 6, 3, 4097):
        assert rp(p, p, None, None, p, 1, 1, 0, 1, per, 1.0, 0, 0, None) != 0 and b"multiple of 4" in err()
    for t in (-1.0, nan, inf, -inf):
        assert rp(p, p, None, None, p, 1, 1, 0, 1, 4, t, 0, 0, None) != 0 and b"temperature" in err()
    for args in ((odd, p, None, None, p), (p, odd, None, None, p), (p, p, odd, None, p), (p, p, None, odd, p), (p, p, None, None, odd)):
        assert rp(*args, 1, 1, 0, 1, 4, 1.0, 0, 0, None) != 0 and b"aligned" in err()

    acc = lib.vcg_sample_accumulate
    q = ctypes.c_void_p(8192)
    assert acc(None, p, q, 1, 1, 0, 16, None) != 0 and b"null" in err()
    assert acc(p, p, None, 1, 1, 0, 16, None) != 0 and b"null" in err()
    assert acc(p, p, q, 0, 1, 0, 16, None) != 0 and b"at least 1" in err()
    assert acc(p, p, q, 1, 0, 0, 16, None) != 0 and b"at least 1" in err()
    assert acc(p, p, q, 1, 1, -1, 16, None) != 0 and b"seen" in err()
    assert acc(p, p, q, 1, 2, 2 ** 24 - 1, 16, None) != 0 and b"seen" in err()
    assert acc(p, p, q, 1, 1, 0, 0, None) != 0 and b"pixels" in err()
    assert acc(odd, p, q, 1, 1, 0, 16, None) != 0 and b"aligned" in err()
    assert acc(p, p, odd, 1, 1, 0, 16, None) != 0 and b"aligned" in err()
    assert acc(p, q, q, 1, 1, 0, 16, None) != 0 and b"one buffer" in err()

    assert lib.vcg_spread_workspace(2, 33, 50) == 2 * 3 * 4 * 8 and lib.vcg_spread_workspace(1, 16, 16) == 16
    assert lib.vcg_spread_workspace(0, 16, 16) == 0 and b"bad N" in err()
    assert lib.vcg_spread_workspace(1, 16, -4) == 0 and b"bad N" in err()
    sp = lib.vcg_spread_display_hw
    big = 1 << 20
    assert sp(None, 2, 2.0, p, p, p, 1, 32, 32, 0, 0, 32, 32, p, big, None) != 0 and b"null" in err()
    assert sp(p, 2, 2.0, p, p, None, 1, 32, 32, 0, 0, 32, 32, p, big, None) != 0 and b"null" in err()
    assert sp(p, 2, 2.0, p, p, p, 1, 32, 32, 0, 0, 32, 32, None, big, None) != 0 and b"null" in err()
    for count in (1, 0, -5):
        assert sp(p, count, 2.0, p, p, p, 1, 32, 32, 0, 0, 32, 32, p, big, None) != 0 and b"at least 2 samples" in err()
    for g in (-0.5, nan, inf):
        assert sp(p, 2, g, p, p, p, 1, 32, 32, 0, 0, 32, 32, p, big, None) != 0 and b"gain" in err()
    assert sp(p, 2, 2.0, p, p, p, 0, 32, 32, 0, 0, 32, 32, p, big, None) != 0 and b"bad N" in err()
    assert sp(p, 2, 2.0, p, p, p, 1, 32, 32, 0, 0, 0, 32, p, big, None) != 0 and b"bad N" in err()
    for top, left, h, w in ((1, 0, 32, 32), (0, -1, 32, 32), (8, 0, 25, 32), (0, 20, 8, 13), (3, 5, 20, 37), (2 ** 31 - 1, 0, 8, 8)):
        assert sp(p, 2, 2.0, p, p, p, 1, 32, 32, top, left, h, w, p, big, None) != 0 and b"leaves" in err()
    assert sp(odd, 2, 2.0, p, p, p, 1, 32, 32, 0, 0, 32, 32, p, big, None) != 0 and b"aligned" in err()
    assert sp(p, 2, 2.0, ctypes.c_void_p(4098), p, p, 1, 32, 32, 0, 0, 32, 32, p, big, None) != 0 and b"aligned" in err()
    assert sp(p, 2, 2.0, p, p, p, 1, 32, 32, 0, 0, 32, 32, odd, big, None) != 0 and b"aligned" in err()
    assert sp(p, 2, 2.0, p, p, p, 2, 48, 64, 0, 0, 33, 50, p, 2 * 3 * 4 * 8 - 1, None) != 0 and b"workspace" in err()
