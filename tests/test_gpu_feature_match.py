"""GPU: the feature-matching kernels (csrc/feature_match.hip, ops.feature_matching) against the float64 restatement of
tests/test_feature_match_host.py.

Shapes: a single row; a pad lane (C = 3 at pitch 4); a discriminator-sized channel count at few rows; the widest discriminator
channel count (two channel groups in the mean kernel); rows one fewer than, equal to, one more than and 2 x + 3 of what one
workgroup takes at a time (ops.fm_chunk: a chunk of float4s in the pair kernels and the backward, a slab of rows in the mean
kernel), at C = 4 and at C = 64; one call with four layers of four different shapes; calls with 1, 2 and 3 layers.

Forward: |got - ref| <= 2^-22 |ref| — summands and sums are in double and rounded once (2^-24); the rest is margin for the
reference's own summation order.  Backward: every element within 1 fp32 ulp of float32(float64(g) coefficient_l), coefficient_l =
1 / (L C_l N H_l W_l), with the reference's sign, exactly 0 where the sign is 0, at upstream g = 1 and g = 0.37; the pad lanes of the
physical gradient buffer are zeros."""
import numpy as np
import pytest
import torch

from test_feature_match_host import MODES, fm_coefficients, fm_reference, fm_signs

pytestmark = pytest.mark.gpu

BASE = [(1, 4, 1, 1), (2, 3, 5, 7), (1, 64, 3, 5), (2, 512, 2, 2)]
FWD_RTOL = 2.0 ** -22


def _edge_shapes(ops, mode):
    """(1, C, 1, rows) with rows around what a workgroup takes at a time, for C = 4 and C = 64."""
    out = []
    for c in (4, 64):
        s = ops.fm_chunk("pair") * 4 // ops.pitch(c) if mode == "pair" else ops.fm_chunk("mean", c)
        assert s >= 2
        out += [(1, c, 1, rows) for rows in (s - 1, s, s + 1, 2 * s + 3)]
    return out


def _cases(ops, mode):
    """lists of layer shapes: every shape alone, then 2, 3 and 4 layers in one call"""
    singles = BASE + _edge_shapes(ops, mode) + _edge_shapes(ops, "mean" if mode == "pair" else "pair")
    return [[s] for s in singles] + [BASE[:2], BASE[:3], BASE, list(reversed(BASE))]


def _nhwc(ops, t, device, grad=False):
    x = ops.to_nhwc(t.to(device)).detach()
    assert ops.can_alias(x)
    return x.requires_grad_(grad)


def _randn(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes], [torch.randn(s, generator=g) for s in shapes]


def _check_forward(got, ref, what):
    got, ref = float(got.detach()), float(ref)
    print(f"{what}: got {got!r} ref {ref!r} rel {abs(got - ref) / max(abs(ref), 1e-300):.3e}")
    assert abs(got - ref) <= FWD_RTOL * abs(ref), f"{what}: {got!r} vs {ref!r}"


def _check_backward(ops, grads, fakes_host, reals_host, mode, g, what):
    coefs = fm_coefficients(fakes_host, g)
    signs = fm_signs(fakes_host, reals_host, mode)
    for i, (grad, coef, sign, f) in enumerate(zip(grads, coefs, signs, fakes_host)):
        assert grad.shape == f.shape and grad.dtype == torch.float32, (what, i)
        got = grad.detach().cpu().double()
        want = sign * coef
        ulp = float(np.spacing(np.float32(abs(coef))))
        zero = sign == 0
        err = (got - want).abs()
        print(f"{what} layer {i}: coefficient {coef!r}, max error {err.max().item():.3e} (ulp {ulp:.3e}), {int(zero.sum())} zeros")
        assert (got[zero] == 0).all(), f"{what} layer {i}: a tie did not get gradient 0"
        assert (err <= ulp).all(), f"{what} layer {i}: {err.max().item():.3e} > one ulp {ulp:.3e}"
        assert (torch.sign(got) == sign).all(), f"{what} layer {i}: wrong sign"
        assert ops.can_alias(grad), f"{what} layer {i}: the gradient is not a view of a physical buffer of the package"
        phys = ops.phys_of(grad)
        c = f.shape[1]
        assert phys.shape[-1] == ops.pitch(c) and (phys[..., c:] == 0).all(), f"{what} layer {i}: pad lanes are not zero"


@pytest.mark.parametrize("mode", MODES)
def test_forward_and_backward_against_float64(mode, pkg, device):
    ops = pkg.ops
    for k, shapes in enumerate(_cases(ops, mode)):
        fh, rh = _randn(shapes, 100 + k)
        fakes = [_nhwc(ops, t, device, grad=True) for t in fh]
        reals = [_nhwc(ops, t, device) for t in rh]
        loss = ops.feature_matching(fakes, reals, mode)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
        what = f"{mode} {shapes}"
        _check_forward(loss, fm_reference(fh, rh, mode), what)
        for g in (1.0, 0.37):
            up = torch.tensor(g, dtype=torch.float32, device=device)
            grads = torch.autograd.grad(loss, fakes, grad_outputs=up, retain_graph=True)
            _check_backward(ops, grads, fh, rh, mode, float(up), f"{what} g={g}")


@pytest.mark.parametrize("mode", MODES)
def test_the_same_call_twice_gives_the_same_bits(mode, pkg, device):
    ops = pkg.ops
    shapes = BASE + _edge_shapes(ops, mode)[3:4]
    for chunk in (shapes[:4], shapes[4:] + shapes[1:3]):
        fh, rh = _randn(chunk, 7)
        outs = []
        for _ in range(2):
            fakes = [_nhwc(ops, t, device, grad=True) for t in fh]
            reals = [_nhwc(ops, t, device) for t in rh]
            loss = ops.feature_matching(fakes, reals, mode)
            outs.append([loss.detach().clone()] + [g.clone() for g in torch.autograd.grad(loss, fakes)])
        for a, b in zip(*outs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_an_equal_block_gets_gradient_zero_in_the_pair_mode(pkg, device):
    ops = pkg.ops
    fh, rh = _randn(BASE, 11)
    rh[1][:, :, 1:4, 2:5] = fh[1][:, :, 1:4, 2:5]
    rh[3][1] = fh[3][1]
    fakes = [_nhwc(ops, t, device, grad=True) for t in fh]
    loss = ops.feature_matching(fakes, [_nhwc(ops, t, device) for t in rh], "pair")
    _check_forward(loss, fm_reference(fh, rh, "pair"), "pair with equal blocks")
    grads = torch.autograd.grad(loss, fakes)
    assert (grads[1][:, :, 1:4, 2:5] == 0).all() and (grads[3][1] == 0).all()
    assert (grads[1][:, :, 0] != 0).all() and (grads[3][0] != 0).all() and (grads[0] != 0).all()
    _check_backward(ops, grads, fh, rh, "pair", 1.0, "pair with equal blocks")


def test_an_equal_channel_gets_a_zero_gradient_column_in_the_mean_mode(pkg, device):
    ops = pkg.ops
    shapes = BASE + [(1, 64, 1, 2 * ops.fm_chunk("mean", 64) + 3)]
    for chunk in (shapes[:4], shapes[4:]):
        fh, rh = _randn(chunk, 12)
        for f, r in zip(fh, rh):
            c = f.shape[1]
            for ch in {0, c // 2, c - 1}:
                r[:, ch] = f[:, ch]
        fakes = [_nhwc(ops, t, device, grad=True) for t in fh]
        loss = ops.feature_matching(fakes, [_nhwc(ops, t, device) for t in rh], "mean")
        _check_forward(loss, fm_reference(fh, rh, "mean"), "mean with equal channels")
        grads = torch.autograd.grad(loss, fakes)
        for f, g in zip(fh, grads):
            c = f.shape[1]
            equal = sorted({0, c // 2, c - 1})
            assert (g[:, equal] == 0).all()
            others = [ch for ch in range(c) if ch not in equal]
            assert not others or (g[:, others] != 0).all()
        _check_backward(ops, grads, fh, rh, "mean", 1.0, "mean with equal channels")


@pytest.mark.parametrize("mode", MODES)
def test_equal_operands_give_exactly_zero(mode, pkg, device):
    ops = pkg.ops
    fh, _ = _randn(BASE + _edge_shapes(ops, mode)[7:8], 13)
    for chunk in (fh[:4], fh[4:]):
        fakes = [_nhwc(ops, t, device, grad=True) for t in chunk]
        reals = [_nhwc(ops, t.clone(), device) for t in chunk]
        loss = ops.feature_matching(fakes, reals, mode)
        assert loss.item() == 0.0
        for g in torch.autograd.grad(loss, fakes):
            assert (g == 0).all() and (ops.phys_of(g) == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_a_contiguous_nchw_operand_gives_the_value_of_its_nhwc_twin(mode, pkg, device):
    """The copy path of as_phys: plain NCHW tensors are converted, and the result has the same bits."""
    ops = pkg.ops
    fh, rh = _randn(BASE, 14)
    twin = ops.feature_matching([_nhwc(ops, t, device, grad=True) for t in fh], [_nhwc(ops, t, device) for t in rh], mode)
    fakes = [t.to(device).requires_grad_(True) for t in fh]
    reals = [t.to(device) for t in rh]
    assert all(t.is_contiguous() for t in fakes) and not ops.can_alias(fakes[1]) and not ops.can_alias(fakes[2])
    loss = ops.feature_matching(tuple(fakes), tuple(reals), mode)
    assert torch.equal(loss.view(torch.int32), twin.view(torch.int32))
    grads = torch.autograd.grad(loss, fakes)
    _check_backward(ops, [ops.to_nhwc(g) for g in grads], fh, rh, mode, 1.0, f"{mode} from NCHW")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("side", ["fake", "real"])
def test_a_nan_in_one_layer_gives_a_nan_loss(mode, side, pkg, device):
    ops = pkg.ops
    fh, rh = _randn(BASE, 15)
    (fh if side == "fake" else rh)[2][0, 17, 1, 3] = float("nan")
    loss = ops.feature_matching([_nhwc(ops, t, device) for t in fh], [_nhwc(ops, t, device) for t in rh], mode)
    assert torch.isnan(loss).item()
    assert not loss.requires_grad                      # nothing wanted a gradient: no graph, no backward launch


def test_only_the_fakes_that_ask_get_a_gradient(pkg, device):
    ops = pkg.ops
    fh, rh = _randn(BASE[1:4], 16)
    for mode in MODES:
        fakes = [_nhwc(ops, t, device, grad=(i != 1)) for i, t in enumerate(fh)]
        reals = [_nhwc(ops, t, device, grad=(i == 0)) for i, t in enumerate(rh)]       # a real that requires grad
        loss = ops.feature_matching(fakes, reals, mode)
        grads = torch.autograd.grad(loss, [fakes[0], fakes[2], reals[0]], allow_unused=True, retain_graph=True)
        assert grads[2] is None                            # the real side is a constant of the term
        signs, coefs = fm_signs(fh, rh, mode), fm_coefficients(fh)
        for got, i in ((grads[0], 0), (grads[1], 2)):
            assert torch.equal(got.cpu().double(), signs[i] * coefs[i])
        loss.backward()
        assert reals[0].grad is None and fakes[1].grad is None and fakes[0].grad is not None


@pytest.mark.parametrize("mode", MODES)
def test_a_second_differentiation_is_refused(mode, pkg, device):
    ops = pkg.ops
    fh, rh = _randn(BASE[:2], 17)
    fakes = [_nhwc(ops, t, device, grad=True) for t in fh]
    loss = ops.feature_matching(fakes, [_nhwc(ops, t, device) for t in rh], mode)
    with pytest.raises(RuntimeError, match="feature_matching: the gradient cannot be differentiated a second time"):
        torch.autograd.grad(loss, fakes, create_graph=True)
