"""GPU: the two kernels of csrc/latent_path.hip (ops.latent_pair_stats, ops.latent_path) against a float64 restatement of the
path, element by element, and the properties the interpolating translator relies on: endpoints that are the inputs' bits, values
that do not depend on the chunking or on the other pairs of a call, pad lanes that are neither summed nor propagated, in-place
reading of two overlapping views of one encoder batch, and the fallback of the slerp to the straight line.

Shapes (C, h, w): 64 x 1 x 1 is less than one workgroup; 64 x 2 x 3 an odd quad count; 6 x 3 x 5 has pitch 8 — two pad lanes per
pixel, which `maps` fills with NaN; 64 x 16 x 16 is the product's 256 px latent; 64 x 40 x 40 gives several workgroups per pair,
so the partial-slot path of the stats runs."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(64, 1, 1), (64, 2, 3), (6, 3, 5), (64, 16, 16), (64, 40, 40)]
PAIRS = (1, 3, 5)
FRACTIONS = (2, 3, 10, 64)
U = 2.0 ** -24                        # the unit roundoff of fp32
MIN_SIN = 1e-4                        # VCG_SLERP_MIN_SIN


def maps(ops, n, shape, seed, scale=1.0):
    """n logical (C, h, w) latent maps in the networks' layout, the pad lanes (if any) full of NaN -> (logical view, physical buffer)."""
    c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    phys = torch.full((n, h, w, ops.pitch(c)), float("nan"))
    phys[..., :c] = torch.randn((n, h, w, c), generator=g) * scale
    phys = phys.to(DEV)
    return ops.logical_of(phys, c), phys


def sums64(a, b):
    """(P, 3) float64 sums over the logical channels and, per pair, the sums of the summands' magnitudes."""
    x, y = a.double().flatten(1), b.double().flatten(1)              # the logical view: no pad lane is in it
    return (torch.stack([(x * x).sum(1), (y * y).sum(1), (x * y).sum(1)], 1).cpu().numpy(),
            torch.stack([(x * x).sum(1), (y * y).sum(1), (x * y).abs().sum(1)], 1).cpu().numpy())


def coefs64(stats, total, mode):
    """The float64 restatement of the coefficients: (P, T, 2)."""
    t = np.arange(total, dtype=np.float64) / (total - 1)
    out = np.empty((len(stats), total, 2))
    for p, (saa, sbb, sab) in enumerate(stats):
        ca, cb = 1.0 - t, t
        if mode == "slerp" and saa > 0 and sbb > 0:
            w = math.acos(min(1.0, max(-1.0, sab / math.sqrt(saa * sbb))))
            if math.sin(w) >= MIN_SIN:
                ca, cb = np.sin((1.0 - t) * w) / math.sin(w), np.sin(t * w) / math.sin(w)
        out[p, :, 0], out[p, :, 1] = ca, cb
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ the stats
@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats_match_float64_sums(pkg, shape, pairs):
    ops = pkg.ops
    a, _ = maps(ops, pairs, shape, 11)
    b, _ = maps(ops, pairs, shape, 12, scale=0.5)
    got = ops.latent_pair_stats(a, b)
    assert got.dtype == torch.float64 and tuple(got.shape) == (pairs, 3) and got.is_cuda
    want, mags = sums64(a, b)
    err = np.abs(got.cpu().numpy() - want)
    print(f"{shape} P={pairs}: worst |error| / sum |summand| {float((err / mags).max()):.3e}")
    assert (err <= 1e-12 * mags).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_pairs_stats_do_not_depend_on_the_other_pairs(pkg, shape):
    ops = pkg.ops
    a, _ = maps(ops, 5, shape, 21)
    b, _ = maps(ops, 5, shape, 22)
    together = ops.latent_pair_stats(a, b)
    for p in range(5):
        alone = ops.latent_pair_stats(a[p:p + 1], b[p:p + 1])
        assert torch.equal(alone.view(torch.int64), together[p:p + 1].view(torch.int64)), p
    assert torch.equal(ops.latent_pair_stats(a, b).view(torch.int64), together.view(torch.int64)), "the same bits on every call"


# ------------------------------------------------------------------ the path against float64
@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_path_matches_the_float64_restatement(pkg, shape, pairs):
    """|z - z64| <= 4 u (|ca a| + |cb b|), u = 2^-24: the coefficients are rounded once (u each, so u on the sum of the two
    magnitudes), cb b is rounded once (u |cb b|) and the fused multiply-add once (u |z| <= u times the same sum): 3 u; the fourth
    covers the device's double-precision acos / sin and summation order against the host's.  coef_out: 2 u relative."""
    ops = pkg.ops
    c, h, w = shape
    a, _ = maps(ops, pairs, shape, 31)
    b, _ = maps(ops, pairs, shape, 32, scale=0.7)
    stats, _ = sums64(a, b)
    a64, b64 = a.double(), b.double()
    worst = 0.0
    for total in FRACTIONS:
        for mode in ops.LATENT_PATH_MODES:
            z, coef = ops.latent_path(a, b, total - 2, mode=mode, return_coef=True)
            assert tuple(z.shape) == (pairs * total, c, h, w) and tuple(coef.shape) == (pairs, total, 2)
            want = coefs64(stats, total, mode)
            assert (np.abs(coef.cpu().numpy().astype(np.float64) - want) <= 2 * U * np.abs(want)).all(), (total, mode)
            cw = torch.from_numpy(want).to(DEV)
            ta = cw[:, :, 0].reshape(pairs, total, 1, 1, 1) * a64[:, None]
            tb = cw[:, :, 1].reshape(pairs, total, 1, 1, 1) * b64[:, None]
            err = (z.double().reshape(pairs, total, c, h, w) - (ta + tb)).abs()
            mag = ta.abs() + tb.abs()
            assert bool((err <= 4 * U * mag).all()), (total, mode, float((err / mag.clamp_min(1e-300)).max()) / U)
            worst = max(worst, float((err / mag.clamp_min(1e-300)).max()) / U)
            zp = ops.phys_of(z)
            assert bool((zp[..., c:] == 0).all()), "pad lanes of z are written as 0"
            zr = z.reshape(pairs, total, c, h, w)
            assert torch.equal(bits(zr[:, 0]), bits(a)) and torch.equal(bits(zr[:, -1]), bits(b)), "the endpoints are the inputs"
            assert torch.equal(coef[:, 0].cpu(), torch.tensor([[1.0, 0.0]] * pairs)) and torch.equal(coef[:, -1].cpu(), torch.tensor([[0.0, 1.0]] * pairs))
    print(f"{shape} P={pairs}: worst |z - z64| / (|ca a| + |cb b|) = {worst:.3f} u (bound 4 u)")


# ------------------------------------------------------------------ properties
def test_endpoints_are_the_bits_of_the_inputs(pkg):
    ops = pkg.ops
    shape = (6, 3, 5)
    a, ap = maps(ops, 2, shape, 41)
    b, bp = maps(ops, 2, shape, 42)
    ap[0, 0, 0, 0], ap[0, 1, 2, 3], ap[1, 2, 4, 5] = -0.0, float("nan"), -0.0
    bp[0, 0, 0, 1], bp[1, 1, 1, 1] = -0.0, torch.tensor(0x7FC01234, dtype=torch.int32).view(torch.float32)   # a NaN with a payload
    for mode in ops.LATENT_PATH_MODES:
        ends = ops.latent_path(a, b, 0, mode=mode)                  # T = 2: just the endpoints
        assert tuple(ends.shape) == (4, 6, 3, 5)
        assert torch.equal(bits(ends[0::2]), bits(a)) and torch.equal(bits(ends[1::2]), bits(b)), mode
        z = ops.latent_path(a, b, 3, mode=mode).reshape(2, 5, 6, 3, 5)
        assert torch.equal(bits(z[:, 0]), bits(a)) and torch.equal(bits(z[:, 4]), bits(b)), mode
        assert bool((ops.phys_of(z.reshape(10, 6, 3, 5))[..., 6:] == 0).all())
        inner = z[:, 1:4]
        assert bool(torch.isnan(inner[0, :, 3, 1, 2]).all()) and bool(torch.isnan(inner[1, :, 1, 1, 1]).all()), "a NaN element stays one"
        assert int(torch.isnan(inner).sum()) == 6, "and reaches no other element: the pairs' NaN stats fall back to the lerp"


@pytest.mark.parametrize("shape", [(6, 3, 5), (64, 40, 40)], ids=lambda s: "x".join(map(str, s)))
def test_chunked_calls_have_the_bits_of_one_call(pkg, shape):
    ops = pkg.ops
    a, _ = maps(ops, 3, shape, 51)
    b, _ = maps(ops, 3, shape, 52)
    total = 10
    for mode in ops.LATENT_PATH_MODES:
        whole, cwhole = ops.latent_path(a, b, total - 2, mode=mode, return_coef=True)
        whole = whole.reshape(3, total, *shape)
        for first, k in ((0, 1), (1, 3), (4, 6)):
            part, cpart = ops.latent_path(a, b, total - 2, mode=mode, first=first, count=k, return_coef=True)
            assert torch.equal(bits(part.reshape(3, k, *shape)), bits(whole[:, first:first + k])), (mode, first, k)
            assert torch.equal(bits(cpart), bits(cwhole[:, first:first + k])), (mode, first, k)


@pytest.mark.parametrize("shape", [(6, 3, 5), (64, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_overlapping_views_of_one_batch_are_read_in_place(pkg, shape):
    ops = pkg.ops
    mu, phys = maps(ops, 4, shape, 61)
    a, b = mu[:-1], mu[1:]
    assert ops.can_alias(a) and ops.can_alias(b)
    assert ops.as_phys(a).data_ptr() == phys.data_ptr() and ops.as_phys(b).data_ptr() == phys[1:].data_ptr(), "nothing is copied"
    ca = ops.logical_of(phys[:-1].clone(), shape[0])
    cb = ops.logical_of(phys[1:].clone(), shape[0])
    assert torch.equal(ops.latent_pair_stats(a, b).view(torch.int64), ops.latent_pair_stats(ca, cb).view(torch.int64))
    for mode in ops.LATENT_PATH_MODES:
        assert torch.equal(bits(ops.latent_path(a, b, 5, mode=mode)), bits(ops.latent_path(ca, cb, 5, mode=mode))), mode


def test_slerp_keeps_the_norm_and_lerp_does_not(pkg):
    ops = pkg.ops
    shape = (64, 16, 16)
    a, ap = maps(ops, 3, shape, 71)
    b, bp = maps(ops, 3, shape, 72, scale=3.0)
    bp *= (ap.flatten(1).norm(dim=1) / bp.flatten(1).norm(dim=1)).view(3, 1, 1, 1)      # equal norms
    norm = a.double().flatten(1).norm(dim=1)
    total = 9
    zs = ops.latent_path(a, b, total - 2, mode="slerp").double().reshape(3, total, -1).norm(dim=2)
    zl = ops.latent_path(a, b, total - 2, mode="lerp").double().reshape(3, total, -1).norm(dim=2)
    assert bool(((zs - norm[:, None]).abs() <= 1e-5 * norm[:, None]).all()), float(((zs - norm[:, None]).abs() / norm[:, None]).max())
    assert bool((zl[:, total // 2] < 0.8 * norm).all()), "the midpoint of the straight line between near-orthogonal maps is ~0.71 of the norm"


def test_fallback_cases_use_the_lerp_coefficients(pkg):
    ops = pkg.ops
    shape = (64, 2, 3)
    a, _ = maps(ops, 1, shape, 81)
    zero = torch.zeros_like(a)
    cases = {"b = a": (a, a.clone()), "b = -a": (a, -a), "a = 0": (zero, a), "b = 0": (a, zero), "a = b = 0": (zero, zero),
             "b = a (1 + 1e-6)": (a, a * (1.0 + 1e-6))}
    for name, (x, y) in cases.items():
        zs, cs = ops.latent_path(x, y, 5, mode="slerp", return_coef=True)
        zl, cl = ops.latent_path(x, y, 5, mode="lerp", return_coef=True)
        assert torch.equal(bits(cs), bits(cl)), name
        assert torch.equal(bits(zs), bits(zl)) and bool(torch.isfinite(zs).all()), name
    t = torch.arange(7, dtype=torch.float64) / 6
    assert torch.equal(cl[0].cpu(), torch.stack([1 - t, t], 1).float()), "(1 - t, t) evaluated in double and rounded once"


def test_orthogonal_maps_at_the_midpoint(pkg):
    ops = pkg.ops
    a, ap = maps(ops, 2, (64, 2, 3), 91)
    b, bp = maps(ops, 2, (64, 2, 3), 92, scale=2.0)
    ap[..., 1::2] = 0                                                  # a lives on the even channels, b on the odd ones: sum a b == 0
    bp[..., 0::2] = 0
    assert bool((ops.latent_pair_stats(a, b)[:, 2] == 0).all())
    _, coef = ops.latent_path(a, b, 1, mode="slerp", return_coef=True)
    mid = coef[:, 1].cpu().double()
    s = math.sin(math.pi / 4)
    assert bool(((mid - s).abs() <= 2 * U * s).all()), mid
    assert torch.equal(coef[:, 1, 0], coef[:, 1, 1])


def test_refusals_on_the_device(pkg):
    ops = pkg.ops
    a, _ = maps(ops, 2, (64, 2, 3), 95)
    b, _ = maps(ops, 3, (64, 2, 3), 96)
    with pytest.raises(RuntimeError, match="two \\(P, C, h, w\\) maps of one shape"):
        ops.latent_path(a, b, 3)
    with pytest.raises(RuntimeError, match="two \\(P, C, h, w\\) maps of one shape"):
        ops.latent_pair_stats(a, b[:, :, :1])
    with pytest.raises(RuntimeError, match="P >= 1"):
        ops.latent_path(a[:0], a[:0], 3)
    for kw in (dict(first=-1), dict(first=4, count=2), dict(count=0)):
        with pytest.raises(RuntimeError, match="fractions"):
            ops.latent_path(a, a, 3, **kw)
    with pytest.raises(RuntimeError, match="steps=-1"):
        ops.latent_path(a, a, -1)
    with pytest.raises(RuntimeError, match="stats must be"):
        ops.latent_path(a, a, 3, stats=torch.zeros(2, 3, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        ops.latent_path(a.double(), a.double(), 3)
