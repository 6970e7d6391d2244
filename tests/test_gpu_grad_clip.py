"""Gradient clipping by global norm inside the fused Adam step: vcg_grad_norm and vcg_adam_step_clipped through the C ABI
(csrc/grad_clip.hip, k_adam<true> in csrc/misc.hip), FusedAdam(max_grad_norm=...) against torch's clip_grad_norm_ + Adam, and
configure_optimizers(clip_grad_norm=...) end to end.

A. The norm kernel against float64 on the CPU: reference norm = grad_scale sqrt(sum (double)g^2), reference coefficient =
   min(1, max_norm / (norm + 1e-6)) in double from the fp32 scalars as the C ABI receives them.  Bound, relative, on out[0] and on
   a coefficient below 1: 2^-22 — the sum of exactly squared terms in double is good to about n 2^-53, then one multiply and one
   square root in double and ONE rounding to fp32 (2^-24); the remaining factor 4 is margin for the double operations.  A
   reference coefficient >= 1 must come back as exactly 1.0f.
B. vcg_adam_step_clipped bit for bit against vcg_adam_step at the scale the clip implies; the skip writes nothing.
C. FusedAdam: three steps with a 30 x gradient spike in the middle against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on
   the CPU; the data-parallel scaling (2 g at grad_scale 1/2 == g at grad_scale 1, bit for bit).
D. Autoencoder and CycleVAEGAN steps: off is today's step bit for bit; a clipped step equals an unclipped one run at
   grad_scale = the reported coefficient; a NaN pixel leaves every parameter and moment as it was.

Adam's first update is -lr sign(g) whatever the scale of g: every test meant to see clipping runs at least two steps or starts
from non-zero moments."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_norm_misc import Out, P, _st

pytestmark = pytest.mark.gpu

GN_CHUNK = 16384                      # floats per workgroup of k_grad_norm_partial (csrc/grad_clip.hip: 256 lanes x 16 float4)
GN_FINAL_THREADS = 256                # lanes of k_grad_norm_final, each summing the slots tid, tid + 256, ...
BIG = GN_FINAL_THREADS * GN_CHUNK + 4 + 1       # 257 slots (one more than the second pass has lanes) and a one-element tail
NORM_SIZES = [1, 2, 3, 4, 5, 7, 1023, GN_CHUNK - 1, GN_CHUNK, GN_CHUNK + 1, BIG]
CONTENT_SIZES = NORM_SIZES[-3:]
BOUND = 2.0 ** -22
SCALES = [1.0, 0.5, 1.0 / 3]
ADAM_CAP = 2048 * 256 * 4             # values one pass of k_adam's grid covers (ew_blocks caps at 2048 blocks; csrc/misc.hip)
ADAM_SIZES = [5, 1023, 2 * ADAM_CAP + 1]
LR, B1, B2, ADAM_EPS = 2e-4, 0.5, 0.999, 1e-8
HUGE = 1e25


def f32(x):
    """the scalar as the C ABI receives it"""
    return float(np.float32(x))


def _lib(pkg):
    return pkg._native.lib()


def _ws(pkg, n, device):
    return torch.full((_lib(pkg).vcg_grad_norm_workspace(n) // 4,), float("nan"), dtype=torch.float32, device=device)


def grad_norm(pkg, g, n, scale, max_norm, ws, device):
    out = Out((4,), device)
    pkg._native.check(_lib(pkg).vcg_grad_norm(P(g), n, scale, max_norm, P(out.t), P(ws), ws.numel() * 4, _st()), "vcg_grad_norm")
    return out.check("vcg_grad_norm out").cpu().numpy().copy()


def sumsq64(a):
    a = a.astype(np.float64)
    return float(np.dot(a, a))


def ref_coef(norm64, max_norm):
    return min(1.0, f32(max_norm) / (norm64 + 1e-6))


def contents(n, kind):
    rng = np.random.default_rng(1000 + n % 997)
    if kind == "randn":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "huge":            # the squares overflow fp32
        return np.full(n, 1e25, dtype=np.float32)
    if kind == "tiny":            # the squares underflow fp32
        return np.full(n, 1e-25, dtype=np.float32)
    if kind == "subnormal":
        bits = rng.integers(1, 1 << 23, n, dtype=np.int64).astype(np.uint32) | (rng.integers(0, 2, n, dtype=np.int64).astype(np.uint32) << 31)
        return bits.view(np.float32)
    if kind == "tiers":           # test_gpu_operand_range.py's idea: the magnitude changes by up to 2^60 every 64 elements
        t = rng.choice([0, 9, 19, 30, 60], size=(n + 63) // 64)
        return (rng.standard_normal(n) * 2.0 ** -np.repeat(t, 64)[:n].astype(np.float64)).astype(np.float32)
    raise KeyError(kind)


def check_against_float64(pkg, device, a, what):
    n = a.size
    g = torch.from_numpy(a).to(device)
    ws = _ws(pkg, n, device)
    total = sumsq64(a)
    worst = 0.0
    for scale in SCALES:
        norm = f32(scale) * math.sqrt(total)
        for mult in (0.5, 1.0, 2.0):
            max_norm = f32(mult * norm)
            out = grad_norm(pkg, g, n, scale, max_norm, ws, device)
            e0 = abs(float(out[0]) - norm) / norm
            coef = ref_coef(norm, max_norm)
            worst = max(worst, e0)
            assert e0 <= BOUND, f"{what} scale {scale} : norm {out[0]!r} vs {norm!r}, off by {e0:.3e} (bound {BOUND:.3e})"
            if coef >= 1.0:
                assert out[1] == np.float32(1.0), f"{what} scale {scale} x{mult}: coefficient {out[1]!r}, reference {coef!r} >= 1"
            else:
                e1 = abs(float(out[1]) - coef) / coef
                worst = max(worst, e1)
                assert e1 <= BOUND and out[1] <= 1.0, f"{what} scale {scale} x{mult}: coefficient {out[1]!r} vs {coef!r}, off by {e1:.3e}"
            assert out[2] == 0.0 and out[3] == 0.0, (what, out)
            again = grad_norm(pkg, g, n, scale, max_norm, ws, device)
            assert out.view(np.int32).tolist() == again.view(np.int32).tolist(), f"{what}: two calls, two results"
    return worst


# ====================================================================================================================== A
@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_of_randn_against_float64(n, pkg, device):
    worst = check_against_float64(pkg, device, contents(n, "randn"), f"randn n={n}")
    print(f"vcg_grad_norm randn n={n}: worst relative error {worst:.3e} (bound {BOUND:.3e})")


@pytest.mark.parametrize("kind", ["huge", "tiny", "subnormal", "tiers"])
def test_norm_of_extreme_contents_against_float64(kind, pkg, device):
    """all 1e25: an implementation that squares in fp32 returns inf; all 1e-25 or subnormal: it returns 0"""
    for n in CONTENT_SIZES:
        a = contents(n, kind)
        assert np.isfinite(a).all() and (a != 0).any()
        if kind in ("huge", "tiny", "subnormal"):
            sq = a.astype(np.float32) * a.astype(np.float32)
            assert np.isinf(sq).all() if kind == "huge" else (sq == 0).all()       # fp32 squares are useless here
        worst = check_against_float64(pkg, device, a, f"{kind} n={n}")
        print(f"vcg_grad_norm {kind} n={n}: worst relative error {worst:.3e} (bound {BOUND:.3e})")


def test_norm_of_zeros_and_of_nothing(pkg, device):
    for n in CONTENT_SIZES + [0, 3]:
        g = torch.zeros(max(n, 4), dtype=torch.float32, device=device)
        out = grad_norm(pkg, g, n, 1.0 / 3, 1.0, _ws(pkg, n, device), device)
        assert out.tolist() == [0.0, 1.0, 0.0, 0.0], (n, out)
    # n == 0 reads nothing: a buffer of NaN behind the pointer changes nothing
    g = torch.full((8,), float("nan"), dtype=torch.float32, device=device)
    assert grad_norm(pkg, g, 0, 1.0, 2.0, _ws(pkg, 0, device), device).tolist() == [0.0, 1.0, 0.0, 0.0]


def test_non_finite_elements_raise_the_flag_and_nothing_else_does(pkg, device):
    n = GN_CHUNK + 3                                          # a size with a tail
    base = contents(n, "randn")
    ws = _ws(pkg, n, device)
    for name, idx, val in (("NaN as the very last element", n - 1, np.nan), ("+Inf in the middle", n // 2, np.inf),
                           ("-Inf at element 0", 0, -np.inf)):
        a = base.copy()
        a[idx] = val
        out = grad_norm(pkg, torch.from_numpy(a).to(device), n, 1.0, 1.0, ws, device)
        assert out[2] == 1.0 and out[3] == 0.0, (name, out)
        assert not np.isfinite(out[0]), (name, out)
    assert grad_norm(pkg, torch.from_numpy(base).to(device), n, 1.0, 1.0, ws, device)[2] == 0.0
    for n in CONTENT_SIZES:
        # finite but enormous: the fp32 norm saturates, the flag stays down and the coefficient is the correctly rounded tiny one
        a = np.full(n, 3e38, dtype=np.float32)
        out = grad_norm(pkg, torch.from_numpy(a).to(device), n, 1.0, 1.0, _ws(pkg, n, device), device)
        norm = math.sqrt(sumsq64(a))
        assert norm > 3.5e38 and out[0] == np.float32(np.inf) and out[2] == 0.0, out
        coef = 1.0 / (norm + 1e-6)
        assert 0.0 < coef < 2.0 ** -126                       # an fp32 subnormal: one step of 2^-149 is the rounding unit
        assert abs(float(out[1]) - coef) <= 2.0 ** -149, (out, coef)


def test_grad_norm_refuses_bad_arguments(pkg, device):
    lib = _lib(pkg)
    n = 1000
    g = torch.ones(n + 4, dtype=torch.float32, device=device)
    out = torch.zeros(8, dtype=torch.float32, device=device)
    ws = torch.zeros(16, dtype=torch.float32, device=device)
    big_n = 4 * GN_CHUNK
    need = lib.vcg_grad_norm_workspace(big_n)

    def bad(match, *args):
        assert lib.vcg_grad_norm(*args) != 0, match
        assert match in lib.vcg_last_error(), (match, lib.vcg_last_error())

    bad(b"null pointer", None, n, 1.0, 1.0, P(out), P(ws), 64, _st())
    bad(b"null pointer", P(g), n, 1.0, 1.0, None, P(ws), 64, _st())
    bad(b"null pointer", P(g), n, 1.0, 1.0, P(out), None, 64, _st())
    for m in (0.0, -1.0, float("nan"), float("inf")):
        bad(b"max_norm", P(g), n, 1.0, m, P(out), P(ws), 64, _st())
    for s in (float("inf"), float("nan")):
        bad(b"grad_scale", P(g), n, s, 1.0, P(out), P(ws), 64, _st())
    bad(b"workspace", P(g), big_n, 1.0, 1.0, P(out), P(ws), need - 1, _st())                   # short (never launched: g is small)
    bad(b"aligned", P(g), n, 1.0, 1.0, P(out), P(ws[1:]), 32, _st())
    bad(b"aligned", P(g[1:]), n, 1.0, 1.0, P(out), P(ws), 64, _st())
    bad(b"aligned", P(g), n, 1.0, 1.0, P(out[1:]), P(ws), 64, _st())
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0                                                       # no refused call wrote anything


# ====================================================================================================================== B
def _adam_inputs(n, step, seed):
    """tests/test_gpu_input_rng_adam.py's draw (restated: that module imports the whole input-pipeline oracle): |g| from 1e-12
    to 1e4, v >= m^2, and per element one of: ordinary, g = m = v = 0, g = +-1e25 (g g overflows fp32), g = 0 with history"""
    g_ = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)
    g = sign * 10.0 ** (torch.rand(n, generator=g_) * 16.0 - 12.0)
    p = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0) * (0.02 + 0.3 * torch.rand(n, generator=g_))
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = torch.randn(n, generator=g_) * 10.0 ** (torch.rand(n, generator=g_) * 8.0 - 6.0)
        v = (m * (1.0 + torch.rand(n, generator=g_))) ** 2
    kind = torch.randint(0, 16, (n,), generator=g_)
    if n >= 4:
        kind[-3:] = torch.tensor([1, 2, 0])
        kind[0] = 1
    g[kind == 1] = 0.0
    m[kind == 1] = 0.0
    v[kind == 1] = 0.0
    g[kind == 2] = HUGE * sign[kind == 2]
    g[kind == 3] = 0.0
    return p.float(), g.float(), m.float(), v.float()


def _adam_scalars(step):
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    return (LR / bc1, B1, B2, 1.0 - B1, 1.0 - B2, ADAM_EPS, math.sqrt(bc2))


def _bits(*outs):
    return [o.check("adam").view(torch.int32).clone() for o in outs]


def _same_bits(a, b, what):
    for name, x, y in zip("pmv", a, b):
        assert torch.equal(x, y), f"{what}: {name} differs in {(x != y).sum().item()} of {x.numel()} elements"


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_clipped_adam_bit_for_bit(n, pkg, device):
    """from non-zero moments at step 3: the clipped launch == vcg_adam_step at grad_scale fl32(grad_scale * clip[1]); with the
    bound far above the norm == vcg_adam_step at the plain grad_scale; with a NaN in g nothing is written"""
    lib = _lib(pkg)
    step = 3
    p0, g0, m0, v0 = _adam_inputs(n, step, 3000 + n % 977)
    g = g0.to(device)
    ws = _ws(pkg, n, device)
    sc = _adam_scalars(step)
    total = sumsq64(g0.numpy())

    def plain(scale):
        p, m, v = (Out((n,), device, fill=t.to(device)) for t in (p0, m0, v0))
        pkg._native.check(lib.vcg_adam_step(P(p.t), P(g), P(m.t), P(v.t), n, *sc, scale, _st()), "vcg_adam_step")
        return _bits(p, m, v)

    def clipped(scale, max_norm, grads=g):
        clip = Out((4,), device)
        p, m, v = (Out((n,), device, fill=t.to(device)) for t in (p0, m0, v0))
        pkg._native.check(lib.vcg_grad_norm(P(grads), n, scale, max_norm, P(clip.t), P(ws), ws.numel() * 4, _st()), "vcg_grad_norm")
        pkg._native.check(lib.vcg_adam_step_clipped(P(p.t), P(grads), P(m.t), P(v.t), n, *sc, scale, P(clip.t), _st()),
                          "vcg_adam_step_clipped")
        return _bits(p, m, v), clip.check("clip").cpu().numpy()

    before = [t.to(device).view(torch.int32) for t in (p0, m0, v0)]
    for scale in (1.0, 1.0 / 3):
        norm = f32(scale) * math.sqrt(total)
        unclipped = plain(scale)
        assert not torch.equal(unclipped[0], before[0])
        for frac in (0.5, 1.0 / 3):
            got, clip = clipped(scale, f32(frac * norm))
            assert abs(float(clip[1]) - frac) < 1e-3 and clip[2] == 0.0, clip
            s = np.float32(np.float32(scale) * clip[1])                  # one fp32 multiply
            _same_bits(got, plain(float(s)), f"n={n} scale={scale} max_norm={frac} x norm")
            assert not torch.equal(got[2], unclipped[2])                  # the clip reached exp_avg_sq
        got, clip = clipped(scale, f32(1000.0 * norm))
        assert clip[1] == np.float32(1.0)
        _same_bits(got, unclipped, f"n={n} scale={scale} max_norm=1000 x norm")
    bad = g0.clone()
    bad[n // 2] = float("nan")
    got, clip = clipped(1.0, 1.0, bad.to(device))
    assert clip[2] == 1.0
    _same_bits(got, before, f"n={n} with a NaN in g")                    # int32 views: no NaN elsewhere could hide a write


def test_clipped_adam_refuses_null_pointers(pkg, device):
    lib = _lib(pkg)
    t = [torch.zeros(8, dtype=torch.float32, device=device) for _ in range(5)]
    sc = _adam_scalars(1)
    for hole in (0, 1, 4):                                                # p, g, clip
        ptrs = [None if i == hole else P(x) for i, x in enumerate(t)]
        assert lib.vcg_adam_step_clipped(*ptrs[:4], 8, *sc, 1.0, ptrs[4], _st()) != 0
        assert b"null pointer" in lib.vcg_last_error()
    assert lib.vcg_adam_step_clipped(*[P(x) for x in t[:4]], 0, *sc, 1.0, P(t[4]), _st()) == 0


# ====================================================================================================================== C
SHAPES = [(5, 3, 3, 3), (5,), (7, 5, 1, 1), (3,), (1,)]                   # 135 + 5 + 35 + 3 + 1 parameters: no multiple of 4


def _fused(pkg, device, init, **kw):
    params = [torch.nn.Parameter(t.clone().to(device)) for t in init]
    return params, pkg.optim.FusedAdam(params, lr=LR, betas=(B1, B2), **kw)


def _spiky_grads():
    gen = torch.Generator().manual_seed(17)
    return [[torch.randn(s, generator=gen) * k for s in SHAPES] for k in (1.0, 30.0, 1.0)]


def test_fused_adam_clipping_matches_torch(pkg, device):
    """parameter and moment bounds: those of tests/test_gpu_parity.py::test_fused_adam_matches_torch_optim_adam (assert_close with
    l2 = 1e-6, mx = 2e-6).  The reported norm against clip_grad_norm_'s total_norm: 1e-6 relative (torch sums per-tensor fp32 norms)."""
    from conftest import assert_close, rel_l2
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen) * 0.1 for s in SHAPES]
    max_norm = 5.0                                                        # the plain steps' norm is about sqrt(179) = 13.4
    mine, opt = _fused(pkg, device, init, max_grad_norm=max_norm)
    free, opt_free = _fused(pkg, device, init)
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    topt = torch.optim.Adam(ref, lr=LR, betas=(B1, B2))
    assert opt.max_grad_norm == max_norm and opt_free.max_grad_norm is None and opt_free.clip_state is None
    for step, grads in enumerate(_spiky_grads()):
        for o, ps in ((opt, mine), (opt_free, free)):
            o.zero_grad()
            for p, g in zip(ps, grads):
                p.grad.copy_(g.to(device))
        for r, g in zip(ref, grads):
            r.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt.step()
        opt_free.step()
        topt.step()
        clip = opt.clip_state.cpu().numpy()
        assert abs(float(clip[0]) - float(total)) <= 1e-6 * float(total), (step, clip, float(total))
        assert clip[1] < 1.0 and clip[2] == 0.0 and clip[3] == 0.0
        assert (float(clip[1]) < 0.02) == (step == 1)                      # the spike is clipped 30 times harder
        st, st_free = opt.state_dict()["state"], opt_free.state_dict()["state"]
        for i, (p, r) in enumerate(zip(mine, ref)):
            assert_close(p.detach(), r.detach(), f"step {step} p{i}", l2=1e-6, mx=2e-6)
            assert_close(st[i]["exp_avg"], topt.state[r]["exp_avg"], f"step {step} m{i}", l2=1e-6, mx=2e-6)
            assert_close(st[i]["exp_avg_sq"], topt.state[r]["exp_avg_sq"], f"step {step} v{i}", l2=1e-6, mx=2e-6)
            # ... and this test can see clipping: the unclipped second moments are nowhere near
            assert rel_l2(st_free[i]["exp_avg_sq"], topt.state[r]["exp_avg_sq"]) > 100 * 1e-6, (step, i)
            assert float(st[i]["step"]) == step + 1
    # the padding between the parameters is zero and stayed zero: the norm over the buffer is the norm over the parameters
    used = torch.zeros(opt.total, dtype=torch.bool)
    for p, o in zip(opt.params, opt.offsets):
        used[o:o + p.numel()] = True
    assert (~used).sum().item() == 9 and opt.flat_grad.cpu()[~used].abs().max().item() == 0.0
    # the checkpoint layout does not know about clipping
    sd, sd_free = opt.state_dict(), opt_free.state_dict()
    assert set(sd) == set(sd_free) and set(sd["state"]) == set(sd_free["state"])
    assert [set(g) for g in sd["param_groups"]] == [set(g) for g in sd_free["param_groups"]]
    assert all(set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} for i in sd["state"])
    assert "max_grad_norm" not in opt.param_groups[0] and "max_grad_norm" not in opt.defaults


def test_fused_adam_refuses_a_bad_bound(pkg, device):
    for bad in (0, 0.0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            pkg.optim.FusedAdam([torch.nn.Parameter(torch.zeros(3, device=device))], max_grad_norm=bad)


def test_data_parallel_scale_is_exact(pkg, device):
    """what a two-rank run does without a process group: the buffer holds the SUM 2 g and grad_scale = 1/2.  The power-of-two
    scale is exact everywhere, so the norm, the coefficient and p, m, v equal those of g at grad_scale 1, bit for bit."""
    gen = torch.Generator().manual_seed(6)
    init = [torch.randn(s, generator=gen) * 0.1 for s in SHAPES]
    pa, a = _fused(pkg, device, init, max_grad_norm=5.0)
    pb, b = _fused(pkg, device, init, max_grad_norm=5.0)
    a.grad_scale = 0.5
    for step, grads in enumerate(_spiky_grads()):
        a.zero_grad()
        b.zero_grad()
        for p, q, g in zip(pa, pb, grads):
            p.grad.copy_((2.0 * g).to(device))
            q.grad.copy_(g.to(device))
        a.step()
        b.step()
        assert torch.equal(a.clip_state.view(torch.int32), b.clip_state.view(torch.int32)), (step, a.clip_state, b.clip_state)
        assert a.clip_state[1].item() < 1.0
        for name in ("flat_param", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), (step, name)


# ====================================================================================================================== D
ARCHS = {"autoencoder": (64, 2), "cyclevaegan": (256, 1)}                 # image size, batch: what test_gpu_parity.py's steps use


def _make(pkg, device, arch, **opt_kw):
    torch.manual_seed(5)
    model = pkg.Networks.Autoencoder() if arch == "autoencoder" else pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False)
    model = model.to(device).train()
    model.configure_optimizers(lr=LR, **opt_kw)
    model.configure_loss()
    pkg.ops.manual_seed(11)                                               # the eps stream of the model's first step
    return model


def _batch(pkg, device, arch, step):
    S, B = ARCHS[arch]
    x, y = pkg.synth.batch(B, S, 20261018, step=step)
    xb = torch.from_numpy(x).to(device)
    return {"x": xb, "y": xb if arch == "autoencoder" else torch.from_numpy(y).to(device)}


def _opts(model):
    return {sfx: getattr(model, "optimizer" + sfx) for sfx in ("", "_G", "_D") if getattr(model, "optimizer" + sfx, None) is not None}


def _state(model):
    """parameters and both moment buffers of every optimizer, as bits"""
    torch.cuda.synchronize()
    return {(sfx, name): getattr(o, name).view(torch.int32).clone() for sfx, o in _opts(model).items()
            for name in ("flat_param", "exp_avg", "exp_avg_sq")}


def _assert_same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs in {(a[k] != b[k]).sum().item()} of {a[k].numel()} elements"


def _run(pkg, device, arch, steps, before_step=None, **opt_kw):
    model = _make(pkg, device, arch, **opt_kw)
    out = []
    for step in range(steps):
        if before_step is not None:
            before_step(model, step)
        m = model.training_step(_batch(pkg, device, arch, step))
        clip = {sfx: o.clip_state.cpu().numpy().copy() for sfx, o in _opts(model).items() if o.clip_state is not None}
        out.append((m, _state(model), clip))
    return out


def _clip_keys(arch):
    sfx = [""] if arch == "autoencoder" else ["_G", "_D"]
    return [k + s for s in sfx for k in ("grad_norm", "grad_skipped")]


@pytest.mark.parametrize("arch", list(ARCHS))
def test_off_is_the_step_as_it_was(arch, pkg, device):
    plain = _run(pkg, device, arch, 2)
    off = _run(pkg, device, arch, 2, clip_grad_norm=0.0)
    for step, ((m0, s0, c0), (m1, s1, c1)) in enumerate(zip(plain, off)):
        assert list(m0) == list(m1) and m0 == m1, (step, m0, m1)
        assert not any(k.startswith("grad_") for k in m1) and c0 == {} and c1 == {}
        _assert_same_state(s0, s1, f"{arch} step {step}, clip_grad_norm=0.0")


@pytest.mark.parametrize("arch", list(ARCHS))
def test_clipped_steps_equal_unclipped_steps_at_the_reported_scale(arch, pkg, device):
    plain = _run(pkg, device, arch, 1)
    loose = _run(pkg, device, arch, 1, clip_grad_norm=1e30)              # the throw-away twin: measures, clips nothing
    _assert_same_state(plain[0][1], loose[0][1], f"{arch}: a bound of 1e30")
    assert all(c[1] == 1.0 and c[2] == 0.0 for c in loose[0][2].values())
    assert {k: v for k, v in loose[0][0].items() if k not in _clip_keys(arch)} == plain[0][0]
    c = 0.5 * min(float(v[0]) for v in loose[0][2].values())            # half the (smaller) norm A will report
    assert c > 0.0
    A = _run(pkg, device, arch, 2, clip_grad_norm=c)
    for step, (m, _, clip) in enumerate(A):
        assert [k for k in m if k.startswith("grad_")] == _clip_keys(arch), list(m)
        for sfx, v in clip.items():
            assert m["grad_norm" + sfx] == float(v[0]) and m["grad_skipped" + sfx] == 0.0 == float(v[2])
            assert v[1] < 1.0 or step > 0                                  # the first step is clipped by construction
        assert {k: v for k, v in m.items() if k not in _clip_keys(arch)}.keys() == plain[0][0].keys()
    assert abs(max(float(v[1]) for v in A[0][2].values()) - 0.5) < 1e-3      # the optimizer with the smaller norm: c is half of it
    assert {k: v for k, v in A[0][0].items() if k not in _clip_keys(arch)} == plain[0][0]      # the losses precede the update

    def scale_like_A(model, step):
        for sfx, o in _opts(model).items():
            o.grad_scale = float(np.float32(A[step][2][sfx][1]))

    Bm = _run(pkg, device, arch, 2, before_step=scale_like_A)
    for step in range(2):
        _assert_same_state(A[step][1], Bm[step][1], f"{arch} step {step}: clipped vs unclipped at the reported coefficient")
    # and the clip reached the second moments: after one step they are not the unclipped run's
    assert all(not torch.equal(A[0][1][k], plain[0][1][k]) for k in A[0][1] if k[1] == "exp_avg_sq")


@pytest.mark.parametrize("arch", list(ARCHS))
def test_a_nan_pixel_skips_the_step(arch, pkg, device):
    model = _make(pkg, device, arch, clip_grad_norm=1.0)
    model.training_step(_batch(pkg, device, arch, 0))                     # non-zero moments: a write would show in all three buffers
    before = _state(model)
    batch = _batch(pkg, device, arch, 1)
    batch["x"] = batch["x"].clone()
    batch["x"][0, 1, 5, 7] = float("nan")
    if arch == "autoencoder":
        batch["y"] = batch["x"]
    m = model.training_step(batch)
    _assert_same_state(before, _state(model), f"{arch}: a step on a batch with a NaN pixel")
    for k in _clip_keys(arch):
        if k.startswith("grad_skipped"):
            assert m[k] == 1.0, m
    m = model.training_step(_batch(pkg, device, arch, 2))                 # and the next clean batch trains
    assert all(m[k] == 0.0 for k in _clip_keys(arch) if k.startswith("grad_skipped")), m
    assert any(not torch.equal(before[k], v) for k, v in _state(model).items())
