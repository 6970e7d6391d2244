"""The input transforms (csrc/input.hip), the Philox stream and vcg_adam_step (csrc/misc.hip) and the layout copies, called one by
one through the C ABI and compared element by element with a plain reference: the numpy oracles of oracle/input_oracle.py (pinned
on Pillow by tests/test_input_pipeline.py) and oracle/device_oracle.py (pinned on the published Philox vectors by
tests/test_rng_host.py), or the header's formula in float64.  Outputs are NaN-prefilled `Out` buffers with a guard band.

A. ColorJitter: the 4096 x 4096 image of all 2^24 RGB triples through vcg_input_prejitter, BIT FOR BIT against
   input_oracle.color_jitter_pil.  17 kernel configurations on 16 oracle evaluations (the hue factors 0.0 and 0.0039 give the same
   integer shift, 0: the oracle's result is computed once for the two).  "Hue alone" runs all four ops with the other factors at
   1.0, which covers brightness / contrast / saturation 1.0 as identities.  The frame sits at an odd arena byte offset and a
   non-zero float-buffer pixel offset, after a small frame whose jitter is DISABLED: that frame must hold level / 255 with a
   correctly rounded division, as ToTensor's (k_u8_to_f4 multiplied by 1.f / 255.f, one ulp off for 126 byte values; fixed with
   __fdiv_rn in this change).
B. vcg_input_resample against input_oracle.resample (float64), every element.  Unquantised tolerance per element:
   4 E + 8 U sum|w_y||w_x||v| / (|sum w_y||sum w_x|), E = the largest |fp32 restatement of the oracle - oracle| over the image,
   U = 2^-24 (oracle/device_oracle.py).  On the six cases of test_input_pipeline.py that bound is 6e-7 .. 1.4e-5, tighter than the
   2e-5 used there, so min(bound, 2e-5) applies to them.  Quantised: every value exactly k / 255, |k - k_ref| <= 1, at most 1 % of
   the values (one value for outputs of fewer than 4096) off the oracle's level; tests/test_rng_host.py checks on the CPU that the
   fp32 restatement itself disagrees on at most 0.5 % of every input used here.
   A float-buffer PIXEL offset >= 2^32 would need a 64 GiB buffer on a shared card and is left out: test_rng_host.py reads the
   places that assemble it instead.  The arena BYTE offset >= 2^32 is run (a 4 GiB arena, freed at the end of its test).
C. The Philox stream bit for bit (vcg_rand_uniform), position arithmetic of vcg_randn / vcg_reparam_fwd, the normal draws against
   float64 Box-Muller of the same words (required: all finite, |got - ref| <= 1e-4), the two ends of u01, and the disjointness of
   the draws of one training / validation step.
D. vcg_adam_step against the header's formula in float64 from the fp32 inputs and scalars as passed: m, v to 3 U of the sum of
   the magnitudes of their terms, p to U |p| + 6 U step_size |m / den|.
E. vcg_nchw_to_nhwc / vcg_nhwc_to_nchw / vcg_fill bitwise; argument refusal of every entry point above.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import test_rng_host as H
from test_gpu_norm_misc import Out, P, U, _st
from test_rng_host import do, io

pytestmark = pytest.mark.gpu


def _lib(pkg):
    return pkg._native.lib()


def _ok(pkg, rc, what):
    pkg._native.check(rc, what)


def _lo_hi(x):
    return int(np.uint32(x & 0xFFFFFFFF).view(np.int32)), int(x >> 32)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ====================================================================================================================== A
UNIT = (1.0, 1.0, 1.0)
ALL_OPS = 0 + 4 * 1 + 16 * 2 + 64 * 3
JITTER_CONFIGS = [      # name, brightness, contrast, saturation, hue, order code
    *[(f"hue{h:+.7f}", *UNIT, h, ALL_OPS) for h in (-0.5, -0.1, -1.0 / 255 - 1e-6, 0.0, 0.0039, 0.1, 0.5)],
    *[(f"saturation{s}", 1.0, 1.0, s, 0.0, 2) for s in (0.35, 1.6, 0.0)],          # 1.0: inside the hue configurations
    *[(f"brightness{b}", b, 1.0, 1.0, 0.0, 0) for b in (0.35, 1.6, 0.0)],
    *[(f"contrast{c}", 1.0, c, 1.0, 0.0, 1) for c in (0.5, 1.3)],
    ("full-a", 1.1337, 0.8211, 1.2719, 0.0831, 1 + 4 * 3 + 16 * 0 + 64 * 2),        # contrast, hue, brightness, saturation
    ("full-b", 0.7423, 1.2903, 0.7105, -0.1417, 2 + 4 * 0 + 16 * 3 + 64 * 1),       # saturation, brightness, hue, contrast
]
_ORACLE_CACHE = {}


def _order(name, code):
    """single-op configurations run that op alone; the others all four in the coded order"""
    return (code,) if name.startswith(("saturation", "brightness", "contrast")) else H.order_of(code)


def _code(order):
    """the kernel always runs four slots: a single op is coded as that op followed by identities of ANOTHER op at factor 1.0"""
    return sum(o << (2 * k) for k, o in enumerate(order))


def all_triples():
    idx = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([idx >> 16, (idx >> 8) & 255, idx & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def _jitter_oracle(img, b, c, s, h, order):
    f = [float(np.float32(v)) for v in (b, c, s, h)]
    key = (f[0], f[1], f[2], io.hue_shift_u8(f[3]), order)
    if key in _ORACLE_CACHE:
        return _ORACLE_CACHE[key]
    ref = io.color_jitter_pil(img, *f, order)
    if order == H.order_of(ALL_OPS) and key[3] == 0:       # hue 0.0 and 0.0039: one oracle evaluation serves both
        _ORACLE_CACHE[key] = ref
    return ref


def test_all_triples_mean_of_L():
    """ImageEnhance.Contrast blends against int(mean(L) + 0.5): on the image of all triples that mean is the same number for the
    kernel's integer reduction and the oracle; pin the oracle's."""
    img = all_triples()
    r = np.arange(256, dtype=np.int64)
    L = (r[:, None, None] * 19595 + r[None, :, None] * 38470 + r[None, None, :] * 7471 + 0x8000) >> 16
    assert int(io._to_L(img).astype(np.int64).sum()) == int(L.sum())
    # 127.5000082: half a level decided by the ninth digit of a 31-bit sum, which only an exact (integer) reduction resolves
    assert int(L.sum()) == 2139095177 and int(float(L.sum()) / L.size + 0.5) == 128


@pytest.mark.parametrize("cfg", JITTER_CONFIGS, ids=[c[0] for c in JITTER_CONFIGS])
def test_color_jitter_on_every_rgb_triple(cfg, pkg, device):
    name, b, c, s, h, code = cfg
    order = _order(name, code)
    if len(order) == 1:                                    # pad the four slots with unit-factor ops that are identities
        op = order[0]
        fill = [o for o in (0, 2, 1) if o != op]           # brightness / saturation / contrast at 1.0
        assert (b if fill[0] == 0 else s if fill[0] == 2 else c) == 1.0
        kcode = _code((op, fill[0], fill[0], fill[0]))
    else:
        kcode = code
    img = all_triples()
    small = H.noise_ramp(77, 5, 7)
    small[0, 0], small[0, 1] = (255, 0, 127), (1, 254, 128)
    small.reshape(-1)[:105] = np.arange(105) * 2 + 1       # odd levels: most of the 126 for which v * (1 / 255) != v / 255
    small.reshape(-1)[40:105] = np.arange(65) * 3 + 60
    npx = 1 << 24
    a_small, a_big = 1, 1 + small.size + 1                 # odd byte offsets
    assert a_small % 2 == 1 and a_big % 2 == 1
    f_small, f_big = 3, 3 + 35 + 2                         # pixel offsets in the float buffer, gaps before and between
    arena = torch.zeros(a_big + npx * 3 + 5, dtype=torch.uint8, device=device)
    arena[a_small:a_small + small.size] = _dev(small.reshape(-1), device)
    arena[a_big:a_big + npx * 3] = _dev(img.reshape(-1), device)
    frames = np.zeros((2, 8), np.int32)
    var = np.zeros((2, 4), np.int32)
    for n, (ao, px, fo) in enumerate(((a_small, 35, f_small), (a_big, npx, f_big))):
        frames[n, 0], frames[n, 1] = _lo_hi(ao)
        frames[n, 2] = px
        frames[n, 3], frames[n, 4] = _lo_hi(fo)
        var[n, 0], var[n, 1] = _lo_hi(fo)
        var[n, 2] = px
    jit = np.zeros((2, 8), np.float32)
    jit[0] = (0.0, 0.5, 0.5, 0.5, 0.3, ALL_OPS, 0, 0)      # disabled: the factors must not matter
    jit[1, :6] = (1.0, b, c, s, h, kcode)
    fbuf = Out((f_big + npx, 4), device)
    dfr, dvar, djit = _dev(frames, device), _dev(var, device), _dev(jit, device)
    _ok(pkg, _lib(pkg).vcg_input_prejitter(P(arena), P(dfr), P(djit), P(dvar), P(fbuf.t), 2, _st()), "vcg_input_prejitter")
    got = fbuf.check(name)
    # nothing outside the two frames is written
    assert torch.isnan(got[:f_small]).all() and torch.isnan(got[f_small + 35:f_big]).all()
    # the disabled frame: ToTensor of the decoded bytes, i.e. a correctly rounded division, pad 0
    want_small = torch.zeros(35, 4, dtype=torch.float32)
    want_small[:, :3] = torch.from_numpy(small.reshape(35, 3).astype(np.float32) / np.float32(255.0))
    assert torch.equal(got[f_small:f_small + 35].cpu(), want_small)
    big = got[f_big:].cpu().numpy()                        # numpy divides; a device-side x / 255.0 may multiply by a reciprocal
    del got, fbuf, arena
    assert (big[:, 3] == 0).all()
    lv = np.rint(big[:, :3] * np.float32(255.0))
    assert lv.min() >= 0 and lv.max() <= 255 and np.array_equal(big[:, :3], lv / np.float32(255.0))   # exactly level / 255 in fp32
    levels = lv.astype(np.uint8).reshape(4096, 4096, 3)
    del big, lv
    ref = _jitter_oracle(img, b, c, s, h, order)
    bad = int((levels != ref).any(-1).sum())
    print(f"jitter {name}: {bad} of 2^24 triples differ")
    assert np.array_equal(levels, ref), (name, bad)


# ====================================================================================================================== B
def _params(rows):
    """rows: [(offset, H, W, box, fh, fv, filt, source kind, quantise)] -> int32 [N][16]"""
    g = np.zeros((len(rows), 16), np.int32)
    for k, (off, Hh, Ww, box, fh, fv, filt, kind, q) in enumerate(rows):
        g[k, 0], g[k, 1] = _lo_hi(off)
        g[k, 2:13] = (Hh, Ww, *box, fh, fv, filt, kind, q)
    return g


def _resample(pkg, device, arena, fsrc, rows, S):
    out = Out((len(rows), S, S, 4), device)
    dg = _dev(_params(rows), device)
    _ok(pkg, _lib(pkg).vcg_input_resample(P(arena), P(fsrc), P(dg), P(out.t), len(rows), S, _st()), "vcg_input_resample")
    return out.check("vcg_input_resample").cpu().numpy()


def _check_float(name, got, src, box, S, fh, fv, filt, cap=None):
    ref = io.resample(src, box, S, bool(fh), bool(fv), filt)
    tol, E = do.resample_tolerance(src, box, S, bool(fh), bool(fv), filt, ref)
    if cap is not None:
        tol = np.minimum(tol, cap)
    err = np.abs(got[..., :3].astype(np.float64) - ref)
    print(f"resample {name}: max err {err.max():.3e}, worst err / tol {np.nanmax(err / tol):.3f}, E {E:.3e}, tol {tol.min():.3e} .. {tol.max():.3e}")
    assert not np.isnan(got).any(), name
    assert (err <= tol).all(), (name, err.max(), float((err / tol).max()))
    assert (got[..., 3] == 0).all(), name


def _check_quantised(name, got, src, box, S, fh, fv, filt):
    assert not np.isnan(got).any(), name
    k = np.rint(got[..., :3] * np.float32(255.0))
    assert np.array_equal(got[..., :3], k.astype(np.float32) / np.float32(255.0)) and k.min() >= 0 and k.max() <= 255, name
    assert (got[..., 3] == 0).all(), name
    kref = io.quantize_u8(io.resample(src, box, S, bool(fh), bool(fv), filt)).astype(np.float64)
    d = np.abs(k - kref)
    off = int((d > 0).sum())
    print(f"resample {name} quantised: {off} of {d.size} values one level off")
    assert d.max() <= 1, (name, d.max())
    assert off <= 0.01 * d.size if d.size >= 4096 else off <= 1, (name, off, d.size)


ALL_SINGLE = H.SINGLE_CASES + H.OLD_SINGLE


@pytest.mark.parametrize("case", ALL_SINGLE, ids=[c[0] for c in ALL_SINGLE])
def test_resample_one_image(case, pkg, device):
    name, Hh, Ww, S, box, fh, fv, filt = case
    old = name.startswith("old")
    src = H.old_case_sources()[int(name[3:])] if old else H.case_source(case)
    off = 3                                                                   # odd
    arena = torch.zeros(off + src.size + 1, dtype=torch.uint8, device=device)
    arena[off:off + src.size] = _dev(src.reshape(-1), device)
    got = _resample(pkg, device, arena, None, [(off, Hh, Ww, box, fh, fv, filt, 0, 0), (off, Hh, Ww, box, fh, fv, filt, 0, 1)], S)
    _check_float(name, got[0], src, box, S, fh, fv, filt, cap=2e-5 if old else None)
    _check_quantised(name, got[1], src, box, S, fh, fv, filt)


def _prejitter_frames(pkg, device, arena, frames, device_jit):
    """frames: [(arena offset, pixel count, fbuf pixel offset)]; returns the float buffer (Out)"""
    total = max(fo + px for _, px, fo in frames)
    fr = np.zeros((len(frames), 8), np.int32)
    var = np.zeros((len(frames), 4), np.int32)
    for n, (ao, px, fo) in enumerate(frames):
        fr[n, 0], fr[n, 1] = _lo_hi(ao)
        fr[n, 2] = px
        fr[n, 3], fr[n, 4] = _lo_hi(fo)
        var[n, 0], var[n, 1] = _lo_hi(fo)
        var[n, 2] = px
    fbuf = Out((total, 4), device)
    dfr, djit, dvar = _dev(fr, device), _dev(device_jit, device), _dev(var, device)      # named: they must outlive the launch
    _ok(pkg, _lib(pkg).vcg_input_prejitter(P(arena), P(dfr), P(djit), P(dvar), P(fbuf.t), len(frames), _st()), "vcg_input_prejitter")
    fbuf.check("vcg_input_prejitter")
    torch.cuda.synchronize()
    return fbuf


def test_resample_mixed_launch_of_17(pkg, device):
    """frame sizes, filters, flips, quantise 0 / 1 and both source kinds in one launch; odd arena offsets; the float4 frames are
    written by vcg_input_prejitter on its own (two jittered, two with their jitter disabled)."""
    cases = H.mix_cases()
    offs, pos = [], 1
    for c in cases:
        offs.append(pos)
        pos += c[6].size
        pos += 1 - pos % 2                                                    # next odd offset
    arena = torch.zeros(pos + 4, dtype=torch.uint8, device=device)
    for c, o in zip(cases, offs):
        assert o % 2 == 1
        arena[o:o + c[6].size] = _dev(c[6].reshape(-1), device)
    frames, jit, fpos, foff = [], [], 5, {}
    for k in H.MIX_FLOAT:
        px = cases[k][6].shape[0] * cases[k][6].shape[1]
        frames.append((offs[k], px, fpos))
        foff[k] = fpos
        fpos += px + 3
        j = H.MIX_JITTER[k]
        jit.append((0.0, 1.3, 0.7, 1.3, 0.1, ALL_OPS, 0, 0) if j is None else (*j, 0, 0))
    fbuf = _prejitter_frames(pkg, device, arena, frames, np.array(jit, np.float32))
    for k in H.MIX_FLOAT:                                                     # vcg_input_prejitter on its own: exactly the oracle's levels / 255
        seen = cases[k][0]
        px = seen.shape[0] * seen.shape[1]
        got = fbuf.t[foff[k]:foff[k] + px].cpu().numpy()
        assert np.array_equal(got[:, :3], seen.reshape(px, 3)) and (got[:, 3] == 0).all(), k
    rows = [(foff[k] if k in H.MIX_FLOAT else offs[k], c[6].shape[0], c[6].shape[1], c[1], c[2], c[3], c[4], int(k in H.MIX_FLOAT), c[5])
            for k, c in enumerate(cases)]
    got = _resample(pkg, device, arena, fbuf.t, rows, H.MIX_S)
    assert len({(c[4], c[5], int(k in H.MIX_FLOAT)) for k, c in enumerate(cases)}) >= 6
    for k, (seen, box, fh, fv, filt, q, _) in enumerate(cases):
        (_check_quantised if q else _check_float)(f"mix{k}", got[k], seen, box, H.MIX_S, fh, fv, filt)


def test_resample_grid_stride_loop(pkg, device):
    """N x S x S = 65 x 256 x 256 > 16384 blocks x 256 threads: every thread takes a second output; 65 different images"""
    cases = H.batch_cases(32, H.BIG_N, 24, 60)
    assert H.BIG_N * H.BIG_S * H.BIG_S > 16384 * 256
    offs, pos = [], 7
    for c in cases:
        offs.append(pos)
        pos += c[0].size
        pos += 1 - pos % 2                                                    # next odd offset
    arena = torch.zeros(pos + 4, dtype=torch.uint8, device=device)
    for c, o in zip(cases, offs):
        assert o % 2 == 1
        arena[o:o + c[0].size] = _dev(c[0].reshape(-1), device)
    rows = [(o, c[0].shape[0], c[0].shape[1], c[1], c[2], c[3], c[4], 0, k % 3 == 2) for k, (c, o) in enumerate(zip(cases, offs))]
    got = _resample(pkg, device, arena, None, rows, H.BIG_S)
    for k, (src, box, fh, fv, filt) in enumerate(cases):
        (_check_quantised if k % 3 == 2 else _check_float)(f"big{k}", got[k], src, box, H.BIG_S, fh, fv, filt)


def test_resample_arena_offset_above_4GiB(pkg, device):
    """the high word of the arena BYTE offset: a frame copied to the end of a 4 GiB + one-frame arena (only that frame is read)"""
    src = H.noise_ramp(99, 40, 52)
    base = (1 << 32) + 1                                                      # odd, high word 1
    arena = torch.empty(base + src.size + 3, dtype=torch.uint8, device=device)
    try:
        arena[:4096].zero_()
        arena[base:base + src.size] = _dev(src.reshape(-1), device)
        decoy = H.noise_ramp(100, 40, 52)                                     # what a dropped high word would read instead
        arena[1:1 + decoy.size] = _dev(decoy.reshape(-1), device)
        box = (3, 5, 30, 41)
        assert _lo_hi(base) == (1, 1)
        got = _resample(pkg, device, arena, None, [(base, 40, 52, box, 1, 0, 0, 0, 0), (base, 40, 52, box, 0, 1, 1, 0, 1)], 37)
        _check_float("4GiB", got[0], src, box, 37, 1, 0, 0)
        _check_quantised("4GiB", got[1], src, box, 37, 0, 1, 1)
    finally:
        del arena
        torch.cuda.empty_cache()


# ====================================================================================================================== C
BIG_SEED = 0x9E3779B97F4A7C15                 # >= 2^32: the key's high word is not zero
CAP = 2048 * 256 * 4                          # values one pass of the grid covers (2048 blocks x 256 threads x 4)


def _draw(pkg, device, fn, n, seed, offset):
    out = Out((n,), device)
    _ok(pkg, getattr(_lib(pkg), fn)(P(out.t), n, seed, offset, _st()), fn)
    return out.check(f"{fn} n={n}")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, (1 << 20) + 3, CAP + 4 * 256 * 3 + 2])
def test_rand_uniform_is_the_philox_stream_bit_for_bit(n, pkg, device):
    for offset in (0, (1 << 32) - 2, (1 << 40) + 12345):                      # the second crosses 2^32 inside the call once n > 8
        got = _draw(pkg, device, "vcg_rand_uniform", n, BIG_SEED, offset).cpu().numpy()
        want = do.uniform_of(do.lib_words(BIG_SEED, offset, (n + 3) // 4)).reshape(-1)[:n]
        assert np.array_equal(got, want), (n, offset, int((got != want).sum()))
    assert not np.array_equal(got, do.uniform_of(do.lib_words(BIG_SEED & 0xFFFFFFFF, offset, (n + 3) // 4)).reshape(-1)[:n])


def test_randn_and_reparam_positions_are_counters(pkg, device):
    """vcg_randn(n, offset = k) == vcg_randn(n + 4 k, offset = 0)[4 k:], also across 2^32, and vcg_reparam_fwd writes the same eps"""
    lib = _lib(pkg)
    for n, k, base in ((1001, 37, 0), (4099, 3, (1 << 32) - 2), (CAP + 7, 5, 11)):
        whole = _draw(pkg, device, "vcg_randn", n + 4 * k, BIG_SEED, base)
        part = _draw(pkg, device, "vcg_randn", n, BIG_SEED, base + k)
        assert torch.equal(part, whole[4 * k:]), (n, k, base)
        mu = torch.linspace(-1, 1, n, device=device)
        lv = torch.linspace(-12, 12, n, device=device)
        eps, z, lvc = Out((n,), device), Out((n,), device), Out((n,), device)
        _ok(pkg, lib.vcg_reparam_fwd(P(mu), P(lv), None, P(eps.t), P(z.t), P(lvc.t), n, BIG_SEED, base + k, _st()), "vcg_reparam_fwd")
        assert torch.equal(eps.check("eps"), part), (n, k, base)
        want = mu.double() + part.double() * torch.exp(0.5 * lv.double().clamp(-10, 10))
        assert ((z.check("z").double() - want).abs() <= 8 * U * (mu.abs().double() + (want - mu.double()).abs()) + 1e-30).all()
        assert torch.equal(lvc.check("lvc"), lv.clamp(-10, 10))


def test_randn_against_float64_box_muller(pkg, device):
    """Required: every draw finite and within 1e-4 of float64 Box-Muller of the same words (u01 with its fp32 rounding is part of
    the stream's definition, oracle/device_oracle.py).  Measured on the MI355X over these 3 x (2^22 + 3) draws with the fast
    __logf / __sincosf: max |got - ref| = 2.04e-6, fifty times inside the requirement."""
    worst = 0.0
    n = (1 << 22) + 3
    for seed, offset in ((BIG_SEED, 0), (H.END_SEED, (1 << 32) - 1000), (7, 1 << 20)):
        got = _draw(pkg, device, "vcg_randn", n, seed, offset).cpu().numpy()
        ref = do.randn_of(do.lib_words(seed, offset, (n + 3) // 4)).reshape(-1)[:n]
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - ref)
        worst = max(worst, float(err.max()))
        print(f"randn seed {seed:#x} offset {offset}: max |got - ref| = {err.max():.3e} at ref {ref[err.argmax()]:.4f}")
        assert err.max() <= 1e-4, (seed, offset, err.max())
        assert abs(ref.mean()) < 3e-3 and abs(ref.std() - 1) < 3e-3             # the reference is a normal sample
    print(f"randn: max |got - ref| over all draws = {worst:.3e}")


def test_randn_at_the_two_ends_of_u01(pkg, device):
    """word >> 8 == 0xFFFFFF gives u == 1.0f exactly (radius 0, log 0); word >> 8 == 0 gives u == 2^-25 (radius ~5.887)"""
    for (ctr, col, word), radius in ((H.END_ONES, 0.0), (H.END_ZEROS, math.sqrt(2 * math.log(2.0 ** 25)))):
        words = do.lib_words(H.END_SEED, ctr, 1)
        assert int(words[0, col]) == word
        got = _draw(pkg, device, "vcg_randn", 4, H.END_SEED, ctr).cpu().numpy()
        ref = do.randn_of(words)[0]
        assert np.isfinite(got).all(), got
        print(f"randn end word {word:#010x}: got {got}, float64 {ref}")
        assert np.abs(got - ref).max() <= 1e-4
        assert abs(math.hypot(got[col], got[col + 1]) - radius) <= 1e-4
        eps, z, lvc = Out((4,), device), Out((4,), device), Out((4,), device)
        zero = torch.zeros(4, device=device)
        _ok(pkg, _lib(pkg).vcg_reparam_fwd(P(zero), P(zero), None, P(eps.t), P(z.t), P(lvc.t), 4, H.END_SEED, ctr, _st()), "vcg_reparam_fwd")
        assert np.array_equal(eps.check("eps").cpu().numpy(), got) and np.array_equal(z.check("z").cpu().numpy(), got)


def _model(pkg, arch, latent, device):
    N = pkg.Networks
    if arch == "vae":
        return N.VariationalAutoencoder(latent_dim=latent), 64, 2
    if arch == "doublevae":
        return N.DoubleVariationalAutoencoder(latent_dim=latent), 64, 2
    return N.CycleVAEGAN(latent_dim=latent, paired=False), 256, 1


@pytest.mark.parametrize("latent", [64, 6])
@pytest.mark.parametrize("arch", ["vae", "cyclevaegan", "doublevae"])
def test_eps_draws_of_one_step_do_not_overlap(arch, latent, pkg, device, monkeypatch):
    """Every device-drawn eps of one training step and one validation step covers its own counters [offset, offset + ceil(n / 4))
    and all of them lie below the stream position afterwards.  latent 6 has a channel pitch of 8: the draw is as long as the
    PHYSICAL buffer, and a reservation made from the logical count (ops.eps_tickets before this change) is shorter than the draw
    that uses it."""
    ops = pkg.ops
    lib = _lib(pkg)
    real = lib.vcg_reparam_fwd
    calls = []

    def spy(mu, lv, eps, eps_out, z, lvc, n, seed, offset, stream):
        if eps is None or getattr(eps, "value", 1) is None:
            calls.append((int(offset), int(n), int(seed)))
        return real(mu, lv, eps, eps_out, z, lvc, n, seed, offset, stream)

    torch.manual_seed(3)
    model, S, B = _model(pkg, arch, latent, device)
    model = model.to(device).train()
    model.configure_optimizers(lr=2e-4)
    model.configure_loss()
    x = ops.rand_uniform((B, 3, S, S), device, seed=21, offset=0)
    y = ops.rand_uniform((B, 3, S, S), device, seed=21, offset=1 << 22)
    ops.inject_eps([])
    ops.manual_seed(0xABCDEF0123)
    monkeypatch.setattr(lib, "vcg_reparam_fwd", spy)
    m = model.training_step({"x": x, "y": y})
    n_train = len(calls)
    model.eval()
    with torch.no_grad():
        model.validation_step({"x": x, "y": y})
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(v == v for v in m.values() if isinstance(v, float)), m
    assert n_train >= 1 and len(calls) > n_train, (n_train, len(calls))
    phys = B * ops.pitch(latent) * (S // 16) ** 2
    assert all(n == phys and seed == 0xABCDEF0123 for _, n, seed in calls), calls
    ranges = sorted((off, off + (n + 3) // 4) for off, n, _ in calls)
    print(f"{arch} latent {latent}: {len(calls)} draws, ranges {ranges}, position {ops._RNG['offset']}")
    for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
        assert a1 <= b0, (arch, latent, ranges)
    assert ranges[-1][1] <= ops._RNG["offset"], (ranges, ops._RNG["offset"])


# ====================================================================================================================== D
ADAM_SIZES = [1, 2, 3, 4, 5, 7, 1023, CAP + 3, 2 * (CAP + 3) + 1]
LR, B1, B2, ADAM_EPS = 2e-4, 0.5, 0.999, 1e-8
HUGE = 1e25                                   # g * g (and (1 - beta2) g * g) overflow fp32


def _adam_inputs(n, step, seed):
    g_ = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)
    g = sign * 10.0 ** (torch.rand(n, generator=g_) * 16.0 - 12.0)            # |g| from 1e-12 to 1e4
    p = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0) * (0.02 + 0.3 * torch.rand(n, generator=g_))
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:                                                                    # v >= m^2, as a second moment is
        m = torch.randn(n, generator=g_) * 10.0 ** (torch.rand(n, generator=g_) * 8.0 - 6.0)
        v = (m * (1.0 + torch.rand(n, generator=g_))) ** 2
    kind = torch.randint(0, 16, (n,), generator=g_)
    if n >= 4:                                                               # every kind also where the scalar tail works
        kind[-3:] = torch.tensor([1, 2, 0])
        kind[0] = 1
    if n in (2, 3):
        kind[-1] = 1
    g[kind == 1] = 0.0                                                        # g == 0, v == 0, m == 0: nothing may move
    m[kind == 1] = 0.0
    v[kind == 1] = 0.0
    g[kind == 2] = HUGE * sign[kind == 2]
    g[kind == 3] = 0.0                                                        # g == 0 with history
    return p.float(), g.float(), m.float(), v.float(), kind


@pytest.mark.parametrize("scale", [1.0, 1.0 / 8, 1.0 / 3], ids=["s1", "s1/8", "s1/3"])
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_step_against_the_formula_in_float64(step, scale, pkg, device):
    """Measured on the MI355X, worst error / tolerance over all sizes: p 0.999, m 0.66 - 0.78, v 0.66 at grad_scale 1 and 1/8 (powers
    of two: g * grad_scale is exact) and v 0.33 at grad_scale 1/3.  This test found the plain fp32 formula MISSING the `v` bound at
    grad_scale = 1/3 (1.19 x, 3.6 U of the terms at n >= 2 097 155): gg = g * grad_scale was rounded before it was squared.  k_adam
    now evaluates the second moment in double, from the unrounded product, wherever that product was rounded at all, and is
    unchanged bit for bit where it was not (grad_scale 1 or a power of two)."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32).item()               # the scalar as the C ABI receives it   # noqa: E731
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    step_size, bc2_sqrt = f32(LR / bc1), f32(math.sqrt(bc2))
    w1, w2, b2, eps, gs = f32(1.0 - B1), f32(1.0 - B2), f32(B2), f32(ADAM_EPS), f32(scale)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    misses = []
    for n in ADAM_SIZES:
        p0, g0, m0, v0, kind = _adam_inputs(n, step, 1000 * step + n % 977)
        p, m, v = (Out((n,), device, fill=t.to(device)) for t in (p0, m0, v0))
        gd = g0.to(device)
        _ok(pkg, _lib(pkg).vcg_adam_step(P(p.t), P(gd), P(m.t), P(v.t), n, step_size, f32(B1), b2, w1, w2, eps, bc2_sqrt, gs, _st()), "vcg_adam_step")
        pn, mn, vn = p.check(f"p n={n}"), m.check(f"m n={n}"), v.check(f"v n={n}")
        assert torch.equal(gd.cpu(), g0)
        P0, G, M0, V0 = (t.to(device).double() for t in (p0, g0, m0, v0))
        gg = G * gs
        Mr = M0 + w1 * (gg - M0)
        Vr = V0 * b2 + w2 * gg * gg
        den = Vr.sqrt() / bc2_sqrt + eps
        Pr = P0 - step_size * (Mr / den)
        fin = (kind != 2).to(device)                                          # where fp32 g * g is finite
        tol_m = 3 * U * (M0.abs() + w1 * gg.abs() + w1 * M0.abs())
        tol_v = 3 * U * (V0.abs() * b2 + w2 * gg * gg)
        tol_p = U * P0.abs() + 6 * U * step_size * (Mr / den).abs()
        for key, got, ref, tol in (("m", mn, Mr, tol_m), ("v", vn, Vr, tol_v), ("p", pn, Pr, tol_p)):
            err = (got.double() - ref).abs()[fin]
            assert not torch.isnan(got[fin]).any(), (key, n)
            r = torch.where(err == 0, torch.zeros_like(err), err / tol[fin])
            if r.numel():
                worst[key] = max(worst[key], r.max().item())
            if not (err <= tol[fin]).all():
                misses.append((key, n, round(r.max().item(), 3)))
        still = (kind == 1).to(device)                                        # g == 0, m == 0, v == 0: exactly no update
        assert torch.equal(pn[still], p0.to(device)[still]) and (mn[still] == 0).all() and (vn[still] == 0).all()
        # g * g overflows: what torch.optim.Adam (CPU) does with s * g for the same elements; no NaN where torch has none
        idx = (kind == 2).nonzero().flatten()[:64]
        if idx.numel():
            tp = torch.nn.Parameter(p0[idx].clone())
            opt = torch.optim.Adam([tp], lr=LR, betas=(B1, B2), eps=ADAM_EPS)
            opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0[idx].clone(), "exp_avg_sq": v0[idx].clone()}
            tp.grad = g0[idx] * torch.tensor(gs, dtype=torch.float32)
            opt.step()
            tm, tv = opt.state[tp]["exp_avg"], opt.state[tp]["exp_avg_sq"]
            gm, gv, gp = mn[idx.to(device)].cpu(), vn[idx.to(device)].cpu(), pn[idx.to(device)].cpu()
            assert torch.isinf(tv).all() and torch.equal(gv, tv)
            assert not torch.isnan(tp).any() and not torch.isnan(gp).any() and not torch.isnan(gm).any()
            assert ((gm.double() - tm.double()).abs() <= 3 * U * tm.double().abs() * 2).all()
            assert torch.equal(gp, tp.detach()) and torch.equal(gp, p0[idx])     # sqrt(inf) in the denominator: no update
    print(f"adam step {step} scale {scale:.4f}: worst err / tol {worst}")
    assert not misses, misses


def test_fused_adam_grad_scale_equals_torch_adam_on_scaled_gradients(pkg, device):
    """FusedAdam.step(grad_scale = s) == torch.optim.Adam fed s * g, to the bounds of test_fused_adam_matches_torch_optim_adam"""
    from conftest import assert_close
    shapes = [(16, 8, 3, 3), (16,), (5, 16, 1, 1), (3,), (1,)]
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen) * 0.1 for s in shapes]
    mine = [torch.nn.Parameter(t.clone().to(device)) for t in init]
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    opt = pkg.optim.FusedAdam(mine, lr=LR, betas=(B1, B2))
    topt = torch.optim.Adam(ref, lr=LR, betas=(B1, B2))
    for step, s in enumerate((1.0 / 8, 1.0 / 3, 0.5, 1.0 / 7)):
        opt.zero_grad()
        for p, r in zip(mine, ref):
            g = torch.randn(r.shape, generator=gen) * 10.0 ** (-6.0 * torch.rand(r.shape, generator=gen))
            p.grad.copy_(g.to(device))
            r.grad = g * torch.tensor(s, dtype=torch.float32)
        opt.step(grad_scale=s)
        topt.step()
        st = opt.state_dict()["state"]
        for i, (p, r) in enumerate(zip(mine, ref)):
            assert_close(p.detach(), r.detach(), f"step {step} p{i}", l2=1e-6, mx=2e-6)
            assert_close(st[i]["exp_avg"], topt.state[r]["exp_avg"], f"step {step} m{i}", l2=1e-6, mx=2e-6)
            assert_close(st[i]["exp_avg_sq"], topt.state[r]["exp_avg_sq"], f"step {step} v{i}", l2=1e-6, mx=2e-6)


# ====================================================================================================================== E
LAYOUT_SHAPES = [(2, 5, 7), (3, 61, 47)]       # N, H, W; the second exceeds 2048 blocks x 256 threads from C = 64 on


@pytest.mark.parametrize("C", [1, 3, 4, 5, 64])
def test_layout_copies_bitwise(C, pkg, device):
    lib = _lib(pkg)
    for Pp in sorted({(C + 3) // 4 * 4, C + 4}):
        for N, Hh, Ww in LAYOUT_SHAPES + ([(2, 300, 301)] if C <= 5 else []):
            total = N * Hh * Ww * Pp
            x = torch.randn(N, C, Hh, Ww, device=device)
            x.view(-1)[:: 7] = float("-0.0")
            nhwc = Out((N, Hh, Ww, Pp), device)
            _ok(pkg, lib.vcg_nchw_to_nhwc(P(x), P(nhwc.t), N, C, Hh, Ww, Pp, _st()), "vcg_nchw_to_nhwc")
            got = nhwc.check(f"nchw_to_nhwc C{C} P{Pp}")
            want = torch.zeros(N, Hh, Ww, Pp, device=device)
            want[..., :C] = x.permute(0, 2, 3, 1)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (C, Pp, N, Hh, Ww)      # pad channels +0.0, data bit for bit
            back = Out((N, C, Hh, Ww), device)
            src = got.clone()
            src[..., C:] = float("nan")                                       # the pad channels must not be read into the result
            _ok(pkg, lib.vcg_nhwc_to_nchw(P(src), P(back.t), N, C, Hh, Ww, Pp, _st()), "vcg_nhwc_to_nchw")
            assert torch.equal(back.check(f"nhwc_to_nchw C{C} P{Pp}").view(torch.int32), x.view(torch.int32)), (C, Pp, N, Hh, Ww)
        assert total > 2048 * 256                                              # the last shape of every C runs the grid-stride loop


@pytest.mark.parametrize("n", [1, 3, 4, 1025, 2048 * 256 + 5, 3 * 2048 * 256 + 1])
def test_fill_bitwise(n, pkg, device):
    for value in (0.0, -0.0, 1.5, float("inf"), 1e-45):
        out = Out((n,), device)
        _ok(pkg, _lib(pkg).vcg_fill(P(out.t), value, n, _st()), "vcg_fill")
        want = torch.full((n,), value, dtype=torch.float32, device=device)
        assert torch.equal(out.check(f"fill n={n}").view(torch.int32), want.view(torch.int32)), (n, value)


def test_entry_points_refuse_bad_arguments(pkg, device):
    """Each call returns its error code and launches nothing: the NaN-prefilled outputs stay untouched.  Only arguments the C
    code checks itself."""
    lib = _lib(pkg)
    st = _st()
    src = H.noise_ramp(1, 8, 8)
    arena = _dev(src.reshape(-1), device)
    params = _dev(_params([(0, 8, 8, (0, 0, 8, 8), 0, 0, 0, 0, 0)]), device)
    out = Out((1, 8, 8, 4), device)
    fr = np.zeros((1, 8), np.int32)
    fr[0, 2] = 64
    var = np.zeros((1, 4), np.int32)
    var[0, 2] = 64
    dfr, dvar = _dev(fr, device), _dev(var, device)
    jit = _dev(np.array([[1, 1.1, 0.9, 1.2, 0.05, ALL_OPS, 0, 0]], np.float32), device)
    fbuf = Out((64, 4), device)
    img = Out((1, 8, 8, 4), device)
    vec = Out((8,), device)
    x = torch.ones(8, device=device)
    bad = {
        "resample arena": lambda: lib.vcg_input_resample(None, None, P(params), P(out.t), 1, 8, st),
        "resample params": lambda: lib.vcg_input_resample(P(arena), None, None, P(out.t), 1, 8, st),
        "resample out": lambda: lib.vcg_input_resample(P(arena), None, P(params), None, 1, 8, st),
        "resample N=0": lambda: lib.vcg_input_resample(P(arena), None, P(params), P(out.t), 0, 8, st),
        "resample N<0": lambda: lib.vcg_input_resample(P(arena), None, P(params), P(out.t), -1, 8, st),
        "resample S=0": lambda: lib.vcg_input_resample(P(arena), None, P(params), P(out.t), 1, 0, st),
        "resample S<0": lambda: lib.vcg_input_resample(P(arena), None, P(params), P(out.t), 1, -8, st),
        "resample S>4096": lambda: lib.vcg_input_resample(P(arena), None, P(params), P(out.t), 1, 4097, st),
        "prejitter arena": lambda: lib.vcg_input_prejitter(None, P(dfr), P(jit), P(dvar), P(fbuf.t), 1, st),
        "prejitter frames": lambda: lib.vcg_input_prejitter(P(arena), None, P(jit), P(dvar), P(fbuf.t), 1, st),
        "prejitter jitter": lambda: lib.vcg_input_prejitter(P(arena), P(dfr), None, P(dvar), P(fbuf.t), 1, st),
        "prejitter var": lambda: lib.vcg_input_prejitter(P(arena), P(dfr), P(jit), None, P(fbuf.t), 1, st),
        "prejitter fbuf": lambda: lib.vcg_input_prejitter(P(arena), P(dfr), P(jit), P(dvar), None, 1, st),
        "prejitter N=0": lambda: lib.vcg_input_prejitter(P(arena), P(dfr), P(jit), P(dvar), P(fbuf.t), 0, st),
        "jitter img": lambda: lib.vcg_input_color_jitter(None, P(jit), 1, 8, st),
        "jitter jitter": lambda: lib.vcg_input_color_jitter(P(img.t), None, 1, 8, st),
        "jitter N=0": lambda: lib.vcg_input_color_jitter(P(img.t), P(jit), 0, 8, st),
        "jitter S=0": lambda: lib.vcg_input_color_jitter(P(img.t), P(jit), 1, 0, st),
        "randn null": lambda: lib.vcg_randn(None, 8, 1, 0, st),
        "uniform null": lambda: lib.vcg_rand_uniform(None, 8, 1, 0, st),
        "reparam mu": lambda: lib.vcg_reparam_fwd(None, P(x), None, P(vec.t), P(vec.t), P(vec.t), 8, 1, 0, st),
        "reparam no eps_out": lambda: lib.vcg_reparam_fwd(P(x), P(x), None, None, P(vec.t), P(vec.t), 8, 1, 0, st),
        "adam p": lambda: lib.vcg_adam_step(None, P(x), P(vec.t), P(vec.t), 8, 1e-3, 0.5, 0.999, 0.5, 0.001, 1e-8, 1.0, 1.0, st),
        "adam g": lambda: lib.vcg_adam_step(P(vec.t), None, P(vec.t), P(vec.t), 8, 1e-3, 0.5, 0.999, 0.5, 0.001, 1e-8, 1.0, 1.0, st),
        "nchw src": lambda: lib.vcg_nchw_to_nhwc(None, P(img.t), 1, 4, 8, 8, 4, st),
        "nchw N=0": lambda: lib.vcg_nchw_to_nhwc(P(x), P(img.t), 0, 4, 8, 8, 4, st),
        "nchw P<C": lambda: lib.vcg_nchw_to_nhwc(P(x), P(img.t), 1, 4, 1, 1, 3, st),
        "nhwc dst": lambda: lib.vcg_nhwc_to_nchw(P(x), None, 1, 4, 1, 1, 4, st),
        "nhwc P<C": lambda: lib.vcg_nhwc_to_nchw(P(x), P(img.t), 1, 4, 1, 1, 3, st),
        "fill null": lambda: lib.vcg_fill(None, 1.0, 8, st),
    }
    for what, call in bad.items():
        rc = call()
        assert rc < 0, (what, rc)
        assert lib.vcg_last_error(), what
    torch.cuda.synchronize()
    for o in (out, fbuf, img, vec):
        assert torch.isnan(o.check("refused call")).all()
    assert torch.equal(x, torch.ones(8, device=device))
    # n == 0 is a valid no-op for the flat entry points
    assert lib.vcg_randn(None, 0, 1, 0, st) == 0 and lib.vcg_fill(None, 1.0, 0, st) == 0
    assert lib.vcg_adam_step(P(vec.t), P(x), P(vec.t), P(vec.t), 0, 1e-3, 0.5, 0.999, 0.5, 0.001, 1e-8, 1.0, 1.0, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(vec.check("n == 0")).all()
