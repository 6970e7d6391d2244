"""GPU: translate.py — the image I/O kernels (csrc/image_io.hip, the windowed metrics of csrc/metrics.hip) bit for bit against
numpy, the generators on rectangles against the oracle, and the public interface (translate_images, the CLI) end to end.

Kernel outputs are prefilled with NaN and followed by a guard band of sentinel words, as in test_gpu_norm_misc.py: an element
a kernel does not write, or one it writes past the end, fails the comparison."""
import argparse
import ctypes
import importlib
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_eval_host", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_eval_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
metrics_ref = _host.metrics_ref

DEV = torch.device("cuda:0")
GUARD = 64
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def tr(pkg):
    return importlib.import_module("vae-cyclegan-implementation_amd.translate")


@pytest.fixture(scope="module")
def ev(pkg):
    return importlib.import_module("vae-cyclegan-implementation_amd.test")


class Out:
    """`nbytes` of output prefilled with NaN words (0xFF bytes: NaN as fp32, 255 as uint8), then GUARD sentinel bytes."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
        self.buf[:nbytes] = 0xFF
        self.buf[nbytes:] = SENTINEL

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def get(self, dtype, shape):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == SENTINEL).all()), "the kernel wrote past the end of its output"
        return self.buf[:self.n].view(dtype).reshape(shape).cpu().numpy()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _frames(n, h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, c), dtype=np.uint8)


def load_ref(u8, hp, wp, top, left):
    """numpy: ToTensor's true division, grey replicated / alpha dropped, numpy.pad(mode="reflect"), zero pad channel."""
    n, h, w, c = u8.shape
    rgb = np.repeat(u8, 3, axis=3) if c == 1 else u8[..., :3]
    f = rgb.astype(np.float32) / np.float32(255.0)
    f = np.pad(f, ((0, 0), (top, hp - h - top), (left, wp - w - left), (0, 0)), mode="reflect")
    return np.concatenate([f, np.zeros((n, hp, wp, 1), np.float32)], axis=3)


# ------------------------------------------------------------------ vcg_image_load
@pytest.mark.parametrize("h,w", [(32, 48), (64, 100), (101, 150), (33, 300), (272, 208), (47, 513)])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 3])
def test_image_load_is_numpy_bit_for_bit(pkg, h, w, c, n):
    lib, ops = pkg._native.lib(), pkg.ops
    u8 = _frames(n, h, w, c, 7 * h + w + c + n)
    hp, wp, top, left = ops.pad_plan(h, w)
    src = torch.from_numpy(u8).to(DEV)
    out = Out(n * hp * wp * 16)
    pkg._native.check(lib.vcg_image_load(_p(src), out.ptr(), n, h, w, c, hp, wp, top, left, None), "vcg_image_load")
    got = out.get(torch.float32, (n, hp, wp, 4))
    want = load_ref(u8, hp, wp, top, left)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{n}x{h}x{w}x{c}"
    # the wrapper: the same buffer as a logical (N, 3, Hp, Wp) batch and the window of the frame inside it
    x, window = ops.image_load(src)
    assert tuple(x.shape) == (n, 3, hp, wp) and window == (top, left, h, w) and ops.is_nhwc_view(x)
    assert np.array_equal(ops.phys_of(x).cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_image_load_divides_and_covers_every_byte_value(pkg):
    """All 256 values: v / 255 (ToTensor), which v * (1 / 255) misses for some of them; a frame off centre, borders of 0..15."""
    lib = pkg._native.lib()
    u8 = (np.arange(40 * 52 * 3, dtype=np.int64) * 37 % 256).astype(np.uint8).reshape(1, 40, 52, 3)
    assert len(np.unique(u8)) == 256
    v = np.arange(256, dtype=np.float32)
    assert (v / np.float32(255.0) != v * (np.float32(1.0) / np.float32(255.0))).any()
    src = torch.from_numpy(u8).to(DEV)
    for hp, wp, top, left in ((48, 64, 0, 12), (48, 64, 8, 0), (55, 67, 15, 0), (40, 52, 0, 0)):
        out = Out(hp * wp * 16)
        pkg._native.check(lib.vcg_image_load(_p(src), out.ptr(), 1, 40, 52, 3, hp, wp, top, left, None), "vcg_image_load")
        want = load_ref(u8, hp, wp, top, left)
        assert np.array_equal(out.get(torch.float32, (1, hp, wp, 4)).view(np.uint32), want.view(np.uint32)), (hp, wp, top, left)


# ------------------------------------------------------------------ vcg_to_display_hw
def display_ref(x, window, uint8):
    top, left, h, w = window
    v = x[:, top:top + h, left:left + w, :3]
    if uint8:
        return np.clip(np.floor(255.0 * v.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)
    return np.clip(v, np.float32(0), np.float32(1))


@pytest.mark.parametrize("n,hp,wp,window", [(1, 48, 64, (3, 5, 40, 52)), (3, 112, 160, (6, 5, 100, 150)), (2, 32, 48, (0, 0, 32, 48)),
                                            (1, 64, 528, (1, 7, 63, 517))])
def test_to_display_hw_is_numpy_bit_for_bit(pkg, n, hp, wp, window):
    lib = pkg._native.lib()
    rng = np.random.RandomState(hp + wp)
    x = (rng.rand(n, hp, wp, 4) * 1.4 - 0.2).astype(np.float32)
    x[0, window[0], window[1], :3] = [0.5 / 255, 1.5 / 255, 254.5 / 255]        # ties of the rounding
    x[..., 3] = np.nan                                                           # the pad channel is not looked at
    xd = torch.from_numpy(x).to(DEV)
    top, left, h, w = window
    for uint8 in (True, False):
        out = Out(n * h * w * 3 * (1 if uint8 else 4))
        pkg._native.check(lib.vcg_to_display_hw(_p(xd), out.ptr(), n, hp, wp, top, left, h, w, int(uint8), None), "vcg_to_display_hw")
        got = out.get(torch.uint8 if uint8 else torch.float32, (n, h, w, 3))
        want = display_ref(x, window, uint8)
        assert np.array_equal(got, want), (window, uint8)


@pytest.mark.parametrize("s", [37, 256])
def test_to_display_hw_equals_to_display_on_squares(pkg, s):
    ops = pkg.ops
    x = ops.to_nhwc(torch.from_numpy((np.random.RandomState(s).rand(2, 3, s, s) * 1.4 - 0.2).astype(np.float32)).to(DEV))
    for uint8 in (True, False):
        assert torch.equal(ops.to_display_hw(x, None, uint8), ops.to_display(x, uint8))


# ------------------------------------------------------------------ vcg_image_metrics_hw
def _pair(n, h, w, seed):
    rng = np.random.RandomState(seed)
    o = (rng.rand(n, 3, h, w) * 1.6 - 0.3).astype(np.float32)
    t = np.clip(rng.rand(n, 3, h, w).astype(np.float32) + 0.05 * rng.randn(n, 3, h, w).astype(np.float32), 0, 1)
    return o, t


def _check_metrics(got, o, t, where):
    """The bounds test_gpu_eval.py holds vcg_image_metrics to against float64."""
    for i in range(o.shape[0]):
        l1, mse, psnr, ssim = metrics_ref(o[i], t[i])
        print(f"{where} image {i}: got {got[i]} want {l1:.9g} {mse:.9g} {psnr:.9g} {ssim:.9g}")
        assert abs(got[i, 0] - l1) <= 1e-6 * l1, (where, got[i], l1)
        assert abs(got[i, 1] - mse) <= 1e-6 * mse, (where, got[i], mse)
        assert abs(got[i, 2] - psnr) <= 1e-5 * abs(psnr) + 1e-5, (where, got[i], psnr)
        assert abs(got[i, 3] - ssim) <= 1e-5, (where, got[i], ssim)


@pytest.mark.parametrize("s", [11, 37, 64, 100, 256])
def test_metrics_hw_equal_metrics_on_squares(pkg, s):
    ops = pkg.ops
    o, t = _pair(3, s, s, s)
    O, T = ops.to_nhwc(torch.from_numpy(o).to(DEV)), ops.to_nhwc(torch.from_numpy(t).to(DEV))
    a, b = ops.image_metrics_hw(O, T), ops.image_metrics(O, T)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ops.image_metrics_hw(O, T, (0, 0, s, s)).view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("hp,wp,window", [(48, 80, None), (11, 200, None), (112, 160, (6, 5, 100, 150)), (64, 64, (3, 20, 50, 11)),
                                          (272, 208, (1, 0, 270, 208)), (96, 96, (40, 40, 16, 32))])
def test_metrics_hw_on_rectangles_and_windows(pkg, hp, wp, window):
    ops, lib = pkg.ops, pkg._native.lib()
    n = 2
    top, left, h, w = window or (0, 0, hp, wp)
    o, t = _pair(n, hp, wp, hp * wp + top)
    O, T = ops.to_nhwc(torch.from_numpy(o).to(DEV)), ops.to_nhwc(torch.from_numpy(t).to(DEV))
    tiles = ((h + 15) // 16) * ((w + 15) // 16)
    ws, res = Out(n * tiles * 16), Out(n * 16)
    pkg._native.check(lib.vcg_image_metrics_hw(_p(ops.phys_of(O)), _p(ops.phys_of(T)), res.ptr(), n, hp, wp, top, left, h, w, ws.ptr(),
                                               n * tiles * 16, None), "vcg_image_metrics_hw")
    got = res.get(torch.float32, (n, 4))
    ws.get(torch.float32, (n, tiles, 4))                                   # the workspace's guard band
    _check_metrics(got, o[:, :, top:top + h, left:left + w], t[:, :, top:top + h, left:left + w], f"{hp}x{wp} {window}")
    assert np.array_equal(ops.image_metrics_hw(O, T, window).cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_metrics_hw_read_nothing_outside_the_window_and_ignore_the_batch(pkg):
    ops = pkg.ops
    window = (6, 5, 100, 150)
    top, left, h, w = window
    o, t = _pair(3, 112, 160, 99)
    clean = ops.image_metrics_hw(torch.from_numpy(o).to(DEV), torch.from_numpy(t).to(DEV), window)
    mask = np.ones((112, 160), bool)
    mask[top:top + h, left:left + w] = False
    o2, t2 = o.copy(), t.copy()
    o2[:, :, mask] = np.nan
    t2[:, :, mask] = np.nan
    O, T = torch.from_numpy(o2).to(DEV), torch.from_numpy(t2).to(DEV)
    dirty = ops.image_metrics_hw(O, T, window)
    assert bool(torch.isfinite(dirty).all())
    assert torch.equal(dirty.view(torch.int32), clean.view(torch.int32))
    alone = ops.image_metrics_hw(O[1:2], T[1:2], window)
    assert torch.equal(alone.view(torch.int32), dirty[1:2].view(torch.int32))
    # the window's own content against a contiguous copy of it: the same bits (same tiles, same order)
    crop = ops.image_metrics_hw(torch.from_numpy(np.ascontiguousarray(o[:, :, top:top + h, left:left + w])).to(DEV),
                                torch.from_numpy(np.ascontiguousarray(t[:, :, top:top + h, left:left + w])).to(DEV))
    assert torch.equal(crop.view(torch.int32), clean.view(torch.int32))


# ------------------------------------------------------------------ generators on rectangles against the oracle
SEED_P = 20261016
SIZES = [(32, 48), (96, 160), (272, 208)]


def _synth_into(pkg, module, prefix):
    shapes = {prefix + k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = pkg.synth.state_dict_like(shapes, SEED_P, bias_std=0.02)
    P = {k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items()}
    module.load_state_dict(P)
    pkg.ops.PARAM_EPOCH[0] += 1
    return P


@pytest.fixture(scope="module")
def models(pkg):
    """architecture -> (model on the device in eval mode, oracle parameters by generator prefix)."""
    N = pkg.Networks
    cache = {}

    def get(arch):
        if arch not in cache:
            torch.manual_seed(5)
            if arch == "autoencoder":
                m = N.Autoencoder()
                P = {"": _synth_into(pkg, m, "ae.")}
            elif arch == "vae":
                m = N.VariationalAutoencoder(latent_dim=64)
                P = {"": _synth_into(pkg, m, "vae.")}
            elif arch == "cyclevaegan":
                m = N.CycleVAEGAN(latent_dim=64, paired=False)
                P = {"G": _synth_into(pkg, m.G, "cvg.G."), "F": _synth_into(pkg, m.F, "cvg.F.")}
            elif arch == "doublevae":
                m = N.DoubleVariationalAutoencoder(latent_dim=64)
                P = {"": _synth_into(pkg, m, "dvae.")}
            cache[arch] = (m.to(DEV).eval(), P)
        return cache[arch]
    return get


def _oracle_run(oracle, arch, direction, P, x, eps):
    """The oracle's forward of one direction, in the dtype of x."""
    cast = lambda Q: {k: v.to(x.dtype) for k, v in Q.items()}
    with torch.no_grad():
        if arch == "autoencoder":
            return oracle.autoencoder_forward(x, cast(P[""]))
        if arch == "vae":
            return oracle.vae_forward(x, cast(P[""]), "", eps.to(x.dtype))[0]
        if arch == "cyclevaegan":
            return oracle.vae_forward(x, cast(P["G" if direction == "a2b" else "F"]), "", eps.to(x.dtype))[0]
        Q, s = cast(P[""]), "B" if direction == "a2b" else "A"           # doublevae: A -> B goes through block B and decoder_B
        z, _, _ = oracle.variational_encoder_block(oracle.encoder(x, Q, "encoder."), Q, f"vae_encoder_block_{s}.", eps.to(x.dtype))
        return oracle.decoder(oracle.s_conv(z, Q, f"vae_decoder_block_{s}.conv."), Q, f"decoder_{s}.")


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("arch,direction", [("autoencoder", "a2b"), ("vae", "a2b"), ("cyclevaegan", "a2b"), ("cyclevaegan", "b2a"),
                                            ("doublevae", "a2b"), ("doublevae", "b2a")])
def test_generators_on_rectangles_match_the_oracle(pkg, oracle, tr, models, arch, direction, h, w):
    """(a) max-abs error within 1e-3 of the output's largest magnitude (the parity suite's bound on outputs); (b) relative L2
    error against the oracle in float64 at most 4x that of the oracle's own fp32 run against it (the suite's "4x PyTorch-CPU
    fp32" rule)."""
    ops = pkg.ops
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    model, P = models(arch)
    x = torch.from_numpy(pkg.synth.uniform((1, 3, h, w), SEED_P, f"x/{h}x{w}"))
    eps = torch.from_numpy(pkg.synth.normal((1, 64, h // 16, w // 16), SEED_P, f"eps/{h}x{w}"))
    if arch != "autoencoder":
        ops.inject_eps([eps])
    try:
        with torch.no_grad():
            got = ops.to_nchw_contiguous(tr.generator_of(model, arch, direction)(ops.to_nhwc(x.to(DEV)))).cpu()
    finally:
        ops.inject_eps([])
    o32 = _oracle_run(oracle, arch, direction, P, x, eps)
    o64 = _oracle_run(oracle, arch, direction, P, x.double(), eps)
    assert tuple(got.shape) == (1, 3, h, w) and bool(torch.isfinite(got).all())
    err_a = float((got - o32).abs().max() / o32.abs().max())
    e_gpu, e_cpu = _rel_l2(got, o64), _rel_l2(o32, o64)
    print(f"{arch} {direction} {h}x{w}: max-abs/amax {err_a:.3e}; rel L2 vs fp64: HIP {e_gpu:.3e}, oracle fp32 {e_cpu:.3e}")
    assert err_a <= 1e-3, f"max-abs error {err_a:.3e} of the output's amax"
    assert e_gpu <= 4 * e_cpu, f"rel L2 vs fp64 {e_gpu:.3e} > 4 x the fp32 oracle's {e_cpu:.3e}"


def test_autoencoder_on_a_768x1024_frame(pkg, oracle, tr, models):
    """The size ops.MAX_TRANSLATE_PIXELS must admit: one whole hypersim frame against the fp32 oracle, bound (a)."""
    ops = pkg.ops
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    assert 768 * 1024 <= ops.MAX_TRANSLATE_PIXELS
    model, P = models("autoencoder")
    x = torch.from_numpy(pkg.synth.uniform((1, 3, 768, 1024), SEED_P, "x/768x1024"))
    got = ops.to_nchw_contiguous(tr.run_generator(model, "autoencoder", ops.to_nhwc(x.to(DEV)))).cpu()
    want = _oracle_run(oracle, "autoencoder", "a2b", P, x, None)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"autoencoder 768x1024: max-abs/amax {err:.3e}")
    assert bool(torch.isfinite(got).all()) and err <= 1e-3


# ------------------------------------------------------------------ the public interface
ARCHS = ["autoencoder", "vae", "aegan", "vaegan", "cycleae", "cyclevae", "cycleaegan", "cyclevaegan"]


def _fresh(pkg, arch, seed=11):
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")
    torch.manual_seed(seed)
    return train.create_model(arch, paired=False, latent_dim=64).to(DEV).eval()


@pytest.mark.parametrize("arch", ARCHS)
def test_256_square_equals_test_translate(pkg, tr, ev, arch):
    ops = pkg.ops
    model = _fresh(pkg, arch)
    u8 = _frames(2, 256, 256, 3, 41)
    x, window = ops.image_load(torch.from_numpy(u8).to(DEV))
    assert window == (0, 0, 256, 256)
    ops.manual_seed(77)
    want = ops.to_display(ev.translate(model, arch, x), uint8=True)
    got = tr.translate_images(model, arch, u8, direction="a2b", eps="sample", seed=77)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 256, 256, 3) and got.device.type == "cuda"
    assert torch.equal(got, want)
    ops.manual_seed(77)
    wantf = ops.to_display(ev.translate(model, arch, x))
    assert torch.equal(tr.translate_images(model, arch, u8, seed=77, return_float=True), wantf)


@pytest.mark.parametrize("arch", ["doubleae", "doublevae"])
def test_256_square_double_models_use_their_translate_methods(pkg, tr, ev, arch):
    ops = pkg.ops
    model = _fresh(pkg, arch)
    u8 = _frames(1, 256, 256, 3, 42)
    x, _ = ops.image_load(torch.from_numpy(u8).to(DEV))
    for direction, method in (("a2b", model.translate_A_to_B), ("b2a", model.translate_B_to_A)):
        ops.manual_seed(5)
        with torch.no_grad():
            want = ops.to_display(method(x), uint8=True)
        assert torch.equal(tr.translate_images(model, arch, u8, direction=direction, seed=5), want), direction
    ops.manual_seed(5)
    recon = ops.to_display(ev.translate(model, arch, x), uint8=True)       # decoder_A(encoder(x)): a reconstruction
    assert not torch.equal(tr.translate_images(model, arch, u8, direction="a2b", seed=5), recon)


def test_b2a_runs_f_and_is_refused_without_one(pkg, tr):
    ops = pkg.ops
    model = _fresh(pkg, "cycleae")
    u8 = _frames(1, 64, 96, 3, 43)
    x, _ = ops.image_load(torch.from_numpy(u8).to(DEV))
    with torch.no_grad():
        f, g = ops.to_display_hw(model.F(x), None, uint8=True), ops.to_display_hw(model.G(x), None, uint8=True)
    assert torch.equal(tr.translate_images(model, "cycleae", u8, direction="b2a"), f)
    assert torch.equal(tr.translate_images(model, "cycleae", u8, direction="a2b"), g)
    assert not torch.equal(f, g)
    with pytest.raises(ValueError, match="one generator"):
        tr.translate_images(_fresh(pkg, "autoencoder"), "autoencoder", u8, direction="b2a")


def test_pad_and_crop_is_what_it_says(pkg, tr):
    """A 100x150 frame: the network run on the numpy-reflect-padded 112x160 frame, cropped — bit for bit."""
    ops = pkg.ops
    model = _fresh(pkg, "autoencoder")
    u8 = _frames(2, 100, 150, 3, 44)
    got = tr.translate_images(model, "autoencoder", u8, return_float=True)
    padded = np.pad(u8, ((0, 0), (6, 6), (5, 5), (0, 0)), mode="reflect")
    assert padded.shape == (2, 112, 160, 3)
    xp = torch.from_numpy(np.ascontiguousarray((padded.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))).to(DEV)
    with torch.no_grad():
        y = ops.to_nchw_contiguous(model(ops.to_nhwc(xp)))
    want = y[:, :, 6:106, 5:155].clamp(0, 1).permute(0, 2, 3, 1).contiguous()
    assert tuple(got.shape) == (2, 100, 150, 3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    u8out = tr.translate_images(model, "autoencoder", u8)
    assert np.array_equal(u8out.cpu().numpy(), np.clip(np.floor(255.0 * want.cpu().numpy().astype(np.float64) + 0.5), 0, 255).astype(np.uint8))


@pytest.mark.parametrize("first,second", [((96, 160), (256, 256)), ((256, 256), (48, 80))])
@pytest.mark.parametrize("arch", ["autoencoder", "vae"])
def test_sizes_that_change_between_calls(pkg, tr, arch, first, second):
    """A, B, A on one model with its lazy-Wf packs: the third call gives the first one's bits, and each result is that
    of a model that has seen nothing else.  96x160 -> 256x256 -> 96x160 is the sequence a user meets; 256x256 -> 48x80 is the
    order in which the first geometry leaves the fp32 Wf block out of most packs (every 3x3 layer of the 16x16 bottleneck runs
    from its planes) and the second one reads it (3x5 maps take the direct kernels): a pack that is not rebuilt is caught here."""
    model = _fresh(pkg, arch, seed=21)
    fa, fb = _frames(1, first[0], first[1], 3, 45), _frames(1, second[0], second[1], 3, 46)
    run = lambda m, f: tr.translate_images(m, arch, f, seed=9, return_float=True)
    a1 = run(model, fa)
    b1 = run(model, fb)
    a2 = run(model, fa)
    assert bool(torch.isfinite(b1).all())
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32))
    assert torch.equal(b1.view(torch.int32), run(_fresh(pkg, arch, seed=21), fb).view(torch.int32))
    assert torch.equal(a1.view(torch.int32), run(_fresh(pkg, arch, seed=21), fa).view(torch.int32))


def test_eps_mean_decodes_mu_and_sample_repeats(pkg, oracle, tr, models):
    ops = pkg.ops
    model, P = models("vae")
    u8 = _frames(1, 96, 160, 3, 47)
    a = tr.translate_images(model, "vae", u8, eps="mean", seed=1, return_float=True)
    ops.manual_seed(999)
    b = tr.translate_images(model, "vae", u8, eps="mean", seed=2, return_float=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    x = torch.from_numpy((u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2).copy())
    want = _oracle_run(oracle, "vae", "a2b", P, x, torch.zeros(1, 64, 6, 10)).clamp(0, 1).permute(0, 2, 3, 1)
    err = float((a.cpu() - want).abs().max() / want.abs().max())
    print(f"eps=mean vs oracle decode of mu: {err:.3e}")
    assert err <= 1e-3
    s1 = tr.translate_images(model, "vae", u8, eps="sample", seed=3, return_float=True)
    s2 = tr.translate_images(model, "vae", u8, eps="sample", seed=3, return_float=True)
    s3 = tr.translate_images(model, "vae", u8, eps="sample", seed=4, return_float=True)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert not torch.equal(s1, s3) and not torch.equal(s1, a)
    assert not ops._EPS_QUEUE                                              # nothing injected is left behind


def test_a_frame_above_the_bound_is_refused_before_any_launch(pkg, tr, models):
    ops, lib = pkg.ops, pkg._native.lib()
    model, _ = models("autoencoder")
    n = ops.MAX_TRANSLATE_PIXELS // (768 * 1024) + 1

    frames = torch.zeros((n, 768, 1024, 3), dtype=torch.uint8)           # on the host: a few tens of MB
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    lib.vcg_profile_enable(1)
    try:
        with pytest.raises(RuntimeError, match=f"MAX_TRANSLATE_PIXELS = {ops.MAX_TRANSLATE_PIXELS}"):
            tr.translate_images(model, "autoencoder", frames)
        need = lib.vcg_profile_read(None, 0)
        buf = ctypes.create_string_buffer(max(int(need), 0) + 16)
        lib.vcg_profile_read(buf, len(buf))
    finally:
        lib.vcg_profile_enable(0)
    assert not buf.value.strip(), f"convolution kernels were launched: {buf.value[:200]}"
    assert torch.cuda.memory_allocated(DEV) == before


def test_cli_end_to_end(pkg, tr, tmp_path):
    from PIL import Image
    ops, utils = pkg.ops, pkg.utils
    rng = np.random.RandomState(48)
    src, tgt = tmp_path / "in", tmp_path / "targets"
    src.mkdir()
    tgt.mkdir()
    files = {"a.png": (100, 150, 3), "b.png": (64, 96, 3), "c.png": (100, 150, 3), "d_grey.png": (64, 96)}
    for name, shape in files.items():
        Image.fromarray(rng.randint(0, 256, shape, dtype=np.uint8)).save(src / name)
        Image.fromarray(rng.randint(0, 256, shape, dtype=np.uint8)).save(tgt / name)
    run = tmp_path / "run"
    run.mkdir()
    model = _fresh(pkg, "vae", seed=31)
    args = argparse.Namespace(architecture="vae", latent_dim=64, paired=False, image_size=256)
    model.configure_optimizers(lr=2e-4)                                   # save_checkpoint writes the optimizer states too
    utils.save_checkpoint(model, 3, 0.25, args, str(run / "best_model.pth"))
    with open(run / "args.json", "w") as f:
        json.dump(vars(args), f)
    out = tmp_path / "out"
    rc = tr.main(["--checkpoint", str(run), "--input", str(src), "--output", str(out), "--targets", str(tgt), "--eps", "mean",
                  "--batch_size", "2"])
    assert rc == 0
    assert sorted(os.listdir(out)) == ["a_translated.png", "b_translated.png", "c_translated.png", "d_grey_translated.png", "metrics.json"]
    loaded, arch = tr.load_generator(run, device=DEV)
    assert arch == "vae"
    rep = json.load(open(out / "metrics.json"))
    assert rep["num_files"] == 4
    rows = {}
    for group in (["a.png", "c.png"], ["b.png"], ["d_grey.png"]):         # the batches the tool forms: equal shapes, at most 2
        frames = [np.asarray(Image.open(src / n)) for n in group]
        u8 = tr.translate_images(loaded, "vae", frames, eps="mean").cpu().numpy()
        y, window = tr.translate_padded(loaded, "vae", frames, eps="mean")
        t, _ = ops.image_load(tr._as_frames([np.asarray(Image.open(tgt / n)) for n in group]).to(DEV))
        m = ops.image_metrics_hw(y, t, window).cpu().double().numpy()
        for k, n in enumerate(group):
            assert np.array_equal(np.asarray(Image.open(out / tr.output_name(n))), u8[k]), n
            rows[n] = m[k]
            for i, key in enumerate(tr.METRIC_NAMES):
                assert rep["per_file"][n][key] == (float(m[k, i]) if math.isfinite(m[k, i]) else None), (n, key)
    mean = np.stack([rows[n] for n in sorted(rows)]).mean(axis=0)
    for i, key in enumerate(tr.METRIC_NAMES):
        assert rep["mean"][key] == pytest.approx(float(mean[i]), rel=1e-12)
    # a bare .pth with explicit arguments, the reference's square resize, one file
    out2 = tmp_path / "out2"
    rc = tr.main(["--checkpoint", str(run / "best_model.pth"), "--architecture", "vae", "--latent_dim", "64", "--input", str(src / "a.png"),
                  "--output", str(out2), "--size", "64", "--eps", "mean", "--suffix", "_64"])
    assert rc == 0 and os.listdir(out2) == ["a_64.png"]
    assert np.asarray(Image.open(out2 / "a_64.png")).shape == (64, 64, 3)
