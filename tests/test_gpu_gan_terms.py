"""GPU: ops.gan_terms (csrc/gan_terms.hip) against float64 — the six scalars of every objective and smoothing, the gradient on
the three routes the models take, the edges (kinks, NaN, +-Inf, |z| = 100, views, bad arguments), and its agreement with the
LSGAN kernels it stands beside.

Bounds, from the kernel's arithmetic (U = 2^-24, fp32's unit roundoff):
  forward   |got - ref| <= U |ref| + 2^-45 mean|summand|.  Every summand is evaluated in double from the exactly converted logit
            and summed in double; the result is rounded to fp32 once, at the store: the first part.  The second covers the double
            sum (at most 17 additions per lane, 6 + 3 across lanes and wavefronts) and libm's exp / log1p, each a few 2^-53 of
            the summands' magnitude — 2^-45 leaves two orders of magnitude.  The logit means use the same bound.
  backward  |got - ref| <= 2 U |ref| per element: the product with the upstream scalars and the division by n are made in double,
            then the one rounding of the store.  No element is excluded: kernel and reference classify the same exactly
            representable logit.
The logits are 3 randn with planted values exactly at 0, +-1, +-100 and the fp32 neighbours of +-1.  One restriction, on the
backward of the logistic objective alone: there the logits at +-100 are left out of the relative check, because the exact
gradient sigmoid(-100) / n = 3.7e-44 / n lies below fp32's smallest normal number 1.2e-38 — the stored value is a subnormal or 0
and no relative bound can hold; `test_logistic_gradient_where_it_underflows` checks those elements against the spacing of the
subnormals instead (2^-150, half of it)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CONFIGS = [("lsgan", 0.0), ("lsgan", 0.1), ("hinge", 0.0), ("logistic", 0.0), ("logistic", 0.1)]
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099)          # around a wavefront, around the workgroup, several strides
PAIRS = [(SIZES[i], SIZES[(i + 1) % len(SIZES)]) for i in range(len(SIZES))] + [(None, 257), (1000, None)]
ONE = np.float32(1.0)
PLANTS = [0.0, 1.0, -1.0, 100.0, -100.0, np.nextafter(ONE, np.float32(2)), np.nextafter(ONE, np.float32(0)),
          np.nextafter(-ONE, np.float32(-2)), np.nextafter(-ONE, np.float32(0))]
NAMES = ("g_real", "g_fake", "d_real", "d_fake", "mean_real", "mean_fake")


def logits(n, seed, big=True):
    """3 randn (fp32) with the planted values at random places; a tensor shorter than the list takes a rotating part of it."""
    if n is None:
        return None
    gen = torch.Generator().manual_seed(20261021 + seed)
    z = 3.0 * torch.randn(n, generator=gen)
    plants = [p for p in PLANTS if big or abs(p) < 50.0]
    plants = plants[seed % len(plants):] + plants[:seed % len(plants)]
    where = torch.randperm(n, generator=gen)[:len(plants)]
    for i, p in zip(where.tolist(), plants):
        z[i] = float(p)
    return z


def sp(t):
    return torch.maximum(t, torch.zeros_like(t)) + torch.log1p(torch.exp(-t.abs()))


def summands(z, fake, objective, s):
    """(G summand, D summand) of float64 logits z on one side: the table of the issue / of include/vcg.h."""
    if objective == "lsgan":
        return ((z - 1.0) ** 2, z ** 2) if fake else (z ** 2, (z - (1.0 - s)) ** 2)
    if objective == "hinge":
        return (-z, torch.relu(1.0 + z)) if fake else (z, torch.relu(1.0 - z))
    if fake:
        return sp(-z), sp(z)
    d = (1.0 - s) * sp(-z)
    return sp(z), (d + s * sp(z) if s != 0.0 else d)            # s = 0 switches the term off, it does not multiply an Inf by 0


def reference(real, fake, objective, s):
    """{name: (float64 value, mean |summand|)}; an absent side: zeros."""
    out = {}
    for side, z in (("real", real), ("fake", fake)):
        if z is None:
            out.update({f"g_{side}": (0.0, 0.0), f"d_{side}": (0.0, 0.0), f"mean_{side}": (0.0, 0.0)})
            continue
        z = z.double()
        g, d = summands(z, side == "fake", objective, s)
        for name, v in ((f"g_{side}", g), (f"d_{side}", d), (f"mean_{side}", z)):
            out[name] = (v.mean().item(), v.abs().mean().item())
    return out


def dev(t, device, grad=False):
    return None if t is None else t.to(device).requires_grad_(grad)


def check_forward(got, ref, what):
    worst = 0.0
    for name, value in zip(NAMES, got):
        want, scale = ref[name]
        value = value.item()
        if math.isinf(want):
            assert value == want, f"{what} {name}: {value} vs {want}"
            continue
        bound = U * abs(want) + 2.0 ** -45 * scale
        err = abs(value - want)
        worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else math.inf))
        assert err <= bound, f"{what} {name}: {value!r} vs {want!r}: error {err:.3e}, bound {bound:.3e}"
    print(f"{what}: worst forward error / bound = {worst:.3f}")


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_forward_against_float64(config, pair, pkg, device):
    real, fake = logits(pair[0], 1), logits(pair[1], 2)
    got = pkg.ops.gan_terms(dev(real, device), dev(fake, device), *config)
    assert len(got) == 6 and all(v.dtype == torch.float32 and v.dim() == 0 for v in got)
    check_forward(got, reference(real, fake, *config), f"{config} {pair}")
    for side, z in (("real", real), ("fake", fake)):
        if z is None:                              # the slots of an absent side are written, as zeros
            assert all(got[NAMES.index(f"{k}_{side}")].item() == 0.0 for k in ("g", "d", "mean"))


# the upstream scalars reach the kernel as the fp32 gradients of ops.weighted_sum: weights that fp32 holds exactly
ROUTES = {"G": (0.75, 1.25, None, None), "D": (None, None, 1.0, 1.5), "both": (0.75, 1.25, 1.0, 1.5)}


def reference_gradients(real, fake, config, weights):
    zs = [None if z is None else z.double().requires_grad_(True) for z in (real, fake)]
    loss = 0.0
    for side, z in enumerate(zs):
        if z is None:
            continue
        g, d = summands(z, side == 1, *config)
        for term, w in ((g, weights[side]), (d, weights[2 + side])):
            if w is not None:
                loss = loss + w * term.mean()
    return torch.autograd.grad(loss, [z for z in zs if z is not None])


def device_gradients(pkg, real, fake, config, weights):
    out = pkg.ops.gan_terms(real, fake, *config)
    picked = [(out[i], w) for i, w in enumerate(weights) if w is not None and (real, fake)[i % 2] is not None]
    loss = pkg.ops.weighted_sum([t for t, _ in picked], [w for _, w in picked])
    return torch.autograd.grad(loss, [z for z in (real, fake) if z is not None])


def check_backward(got, want, what):
    worst = 0.0
    for g, r in zip(got, want):
        assert g.dtype == torch.float32 and g.shape == r.shape
        err = (g.double().cpu() - r).abs()
        bound = 2.0 * U * r.abs()
        bad = err > bound
        ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        worst = max(worst, ratio.max().item())
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements off, worst error / bound = {ratio.max().item():.3f} "
                               f"at index {int(ratio.argmax())}: {g.flatten()[int(ratio.argmax())].item()!r} vs {r.flatten()[int(ratio.argmax())].item()!r}")
    print(f"{what}: worst gradient error / bound = {worst:.3f}")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("pair", [(1, 2), (64, 65), (257, 1000), (4099, 255), (None, 257), (1000, None)], ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_backward_against_float64_autograd(config, pair, route, pkg, device):
    big = config[0] != "logistic"                  # see the module docstring
    real, fake = logits(pair[0], 3, big), logits(pair[1], 4, big)
    got = device_gradients(pkg, dev(real, device, True), dev(fake, device, True), config, ROUTES[route])
    want = reference_gradients(real, fake, config, ROUTES[route])
    check_backward(got, want, f"{config} {pair} route {route}")


def test_the_two_phases_of_a_step_share_one_forward(pkg, device):
    """_alternating_step differentiates G_loss with retain_graph, then D_loss, through the same gan_terms node: each call has
    only its own upstream scalars set and gives the bits of a graph that is differentiated once."""
    ops = pkg.ops
    for config in CONFIGS:
        real, fake = dev(logits(257, 5), device, True), dev(logits(1000, 6), device, True)
        out = ops.gan_terms(real, fake, *config)
        g_loss = ops.weighted_sum([out[0], out[1]], [0.75, 1.25])
        d_loss = ops.weighted_sum([out[2], out[3]], [1.0, 1.5])
        g_phase = torch.autograd.grad(g_loss, [real, fake], retain_graph=True)
        d_phase = torch.autograd.grad(d_loss, [real, fake])
        for got, route in ((g_phase, "G"), (d_phase, "D")):
            alone = device_gradients(pkg, real, fake, config, ROUTES[route])
            assert all(torch.equal(a, b) for a, b in zip(got, alone)), (config, route)


def test_a_side_without_an_upstream_gradient_gets_none(pkg, device):
    """VAEGAN's D phase differentiates the real term alone, the generator phase of the cycle models the fake terms alone: the
    other side's logits get no gradient at all (not a tensor of zeros), so autograd does not walk their discriminator pass."""
    real, fake = dev(logits(64, 7), device, True), dev(logits(65, 8), device, True)
    out = pkg.ops.gan_terms(real, fake, "hinge")
    g_real, g_fake = torch.autograd.grad(out[2], [real, fake], retain_graph=True, allow_unused=True)
    assert g_fake is None and g_real is not None and g_real.abs().sum().item() > 0
    g_real, g_fake = torch.autograd.grad(out[1], [real, fake], retain_graph=True, allow_unused=True)
    assert g_real is None and torch.equal(g_fake, torch.full_like(g_fake, -1.0 / 65))
    assert not out[4].requires_grad and not out[5].requires_grad          # the means are not differentiable


def test_the_hinge_gradient_at_the_kinks_is_exactly_zero(pkg, device):
    up, down = np.nextafter(ONE, np.float32(2)), np.nextafter(ONE, np.float32(0))
    real = torch.tensor([1.0, float(down), float(up), 0.0, 3.0, -100.0, 100.0], device=device, requires_grad=True)
    fake = torch.tensor([-1.0, float(-down), float(-up), 0.0, -3.0, 100.0, -100.0], device=device, requires_grad=True)
    out = pkg.ops.gan_terms(real, fake, "hinge")
    g_real, g_fake = torch.autograd.grad(pkg.ops.weighted_sum([out[2], out[3]], [1.0, 1.0]), [real, fake])
    w = float(np.float32(1.0) / np.float32(7.0))                           # 1 / n, rounded once
    assert g_real.tolist() == [0.0, -w, 0.0, -w, 0.0, -w, 0.0]            # max(0, 1 - z): slope -1 below the kink, 0 at and above it
    assert g_fake.tolist() == [0.0, w, 0.0, w, 0.0, w, 0.0]               # max(0, 1 + z): slope 1 above -1, 0 at and below it


def test_logistic_gradient_where_it_underflows(pkg, device):
    """|z| = 100 under the logistic objective: the saturated side's gradient is sigmoid(-100) / n = 3.7e-44 / n, a subnormal of
    fp32 or 0.  Held to the relative bound plus half the subnormal spacing, 2^-150; the other side's is 1 / n to the bound."""
    z = torch.tensor([100.0, -100.0, 0.0, 1.0], dtype=torch.float32)
    for s in (0.0, 0.1):
        got = device_gradients(pkg, dev(z, device, True), dev(z, device, True), ("logistic", s), ROUTES["both"])
        want = reference_gradients(z, z, ("logistic", s), ROUTES["both"])
        for g, r in zip(got, want):
            assert torch.isfinite(g).all()
            err = (g.double().cpu() - r).abs()
            assert (err <= 2.0 * U * r.abs() + 2.0 ** -150).all(), (s, g.tolist(), r.tolist())


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_nan_in_gives_nan_out(config, pkg, device):
    for side in (0, 1):
        zs = [logits(257, 9), logits(65, 10)]
        zs[side][3] = float("nan")
        out = [v.item() for v in pkg.ops.gan_terms(dev(zs[0], device), dev(zs[1], device), *config)]
        for i, name in enumerate(NAMES):
            assert math.isnan(out[i]) == (i % 2 == side), f"{config}: NaN in side {side}: {name} = {out[i]}"


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_infinite_logits_give_the_limit(config, pkg, device):
    """One +Inf or one -Inf logit on a side: every term is the float64 formula's value — finite where the summand's limit is 0
    (the saturated hinge and softplus), +-Inf elsewhere, and never the NaN of an Inf - Inf or 0 x Inf inside the kernel."""
    for side in (0, 1):
        for inf in (float("inf"), -float("inf")):
            zs = [logits(64, 11), logits(1000, 12)]
            zs[side][5] = inf
            got = pkg.ops.gan_terms(dev(zs[0], device), dev(zs[1], device), *config)
            assert not any(math.isnan(v.item()) for v in got), (config, side, inf, [v.item() for v in got])
            check_forward(got, reference(zs[0], zs[1], *config), f"{config} side {side} {inf}")


def test_views_give_the_dense_tensors_bits(pkg, device):
    ops = pkg.ops
    base = dev(logits(2 * 257, 13), device, True)
    grid = dev(logits(12 * 7, 14), device).reshape(12, 7)
    for config in CONFIGS:
        strided, transposed = base[::2], grid.t()
        assert not strided.is_contiguous() and not transposed.is_contiguous()
        out = ops.gan_terms(strided, transposed, *config)
        dense_real = strided.detach().contiguous().requires_grad_(True)
        dense = ops.gan_terms(dense_real, transposed.contiguous(), *config)
        assert all(torch.equal(a, b) for a, b in zip(out, dense)), config
        (g_base,) = torch.autograd.grad(ops.weighted_sum([out[0], out[2]], [1.0, 1.0]), [base])
        (g_dense,) = torch.autograd.grad(ops.weighted_sum([dense[0], dense[2]], [1.0, 1.0]), [dense_real])
        assert torch.equal(g_base[::2], g_dense) and not g_base[1::2].any(), config
        scalar = torch.tensor([[0.625]], device=device)
        expanded = scalar.expand(8, 5)                                      # stride 0 in both dimensions
        assert expanded.stride() == (0, 0)
        out = ops.gan_terms(expanded, None, *config)
        dense = ops.gan_terms(torch.full((8, 5), 0.625, device=device), None, *config)
        assert all(torch.equal(a, b) for a, b in zip(out, dense)), config


def test_bad_arguments_raise(pkg, device):
    ops = pkg.ops
    z = torch.zeros(8, device=device)
    with pytest.raises(RuntimeError, match="objective"):
        ops.gan_terms(z, z, "wgan")
    for smooth in (-0.1, 0.5, float("nan"), True):
        with pytest.raises(RuntimeError, match="smooth"):
            ops.gan_terms(z, z, "logistic", smooth)
    with pytest.raises(RuntimeError, match="hinge"):
        ops.gan_terms(z, z, "hinge", 0.1)
    with pytest.raises(RuntimeError, match="both None"):
        ops.gan_terms(None, None, "lsgan")
    with pytest.raises(RuntimeError, match="float32"):
        ops.gan_terms(z.double(), z, "hinge")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gan_terms(z, z.cpu(), "hinge")
    with pytest.raises(RuntimeError, match="empty"):
        ops.gan_terms(z[:0], z, "hinge")


def test_a_second_differentiation_is_refused(pkg, device):
    z = dev(logits(64, 15), device, True)
    out = pkg.ops.gan_terms(z, None, "logistic")
    with pytest.raises(RuntimeError, match="cannot be differentiated a second time"):
        torch.autograd.grad(out[2], [z], create_graph=True, retain_graph=True)
    (g,) = torch.autograd.grad(out[2], [z])                                 # the first derivative is still there
    assert torch.isfinite(g).all() and g.abs().sum().item() > 0


def test_lsgan_agrees_with_the_four_mse_const_calls(pkg, device):
    """objective lsgan, no smoothing, is the arithmetic of the default path's kernels up to their fp32 square: within
    5 U ref, tests/test_gpu_norm_misc.py::test_mse_const's own forward bound (the logit means: both are double sums, U ref + the
    sum's share)."""
    ops = pkg.ops
    for n_real, n_fake in ((1, 2), (65, 256), (4099, 1000)):
        real, fake = logits(n_real, 16), logits(n_fake, 17)
        ref = reference(real, fake, "lsgan", 0.0)
        r, f = dev(real, device), dev(fake, device)
        fused = ops.gan_terms(r, f, "lsgan")
        four = {"g_real": ops.mse_const(r, 0.0), "g_fake": ops.mse_const(f, 1.0), "d_real": ops.mse_const(r, 1.0), "d_fake": ops.mse_const(f, 0.0)}
        for name, (term, mean) in four.items():
            want = ref[name][0]
            err = abs(fused[NAMES.index(name)].item() - term.item())
            print(f"lsgan {name} n {n_real}x{n_fake}: fused - mse_const = {err / (5 * U * want):.3f} of the bound")
            assert err <= 5 * U * want, (name, fused[NAMES.index(name)].item(), term.item())
            side = "mean_" + name[2:]
            assert abs(fused[NAMES.index(side)].item() - mean.item()) <= 2 * (U * abs(ref[side][0]) + 2.0 ** -45 * ref[side][1])


def test_two_calls_give_the_same_bits(pkg, device):
    for config in CONFIGS:
        real, fake = logits(4099, 18), logits(1000, 19)
        runs = []
        for _ in range(2):
            r, f = dev(real, device, True), dev(fake, device, True)
            out = pkg.ops.gan_terms(r, f, *config)
            grads = torch.autograd.grad(pkg.ops.weighted_sum(list(out[:4]), [0.75, 1.25, 1.0, 1.5]), [r, f])
            runs.append([v.clone() for v in out] + list(grads))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), config
