"""GPU: the multi-scale gradient-matching loss (csrc/grad_loss.hip, ops.grad_match_loss; lambda_grad / grad_scales of the four
models: section 5, bodies in test_gpu_image_terms.py) against a float64 torch restatement of its definition, differentiated by
torch autograd on the CPU: strided slicing,
`.abs().mean()` per direction and scale, a direction without a pair contributing 0, the sum divided by the number of scales.

Bounds.  The kernel forms d = a - b and the pair differences in double (exact for fp32 inputs) and sums in double, so the loss
carries the two conversions to fp32 only: 1e-6 relative.  A gradient element is a sum of at most 16 sign terms, each rounded once
in fp32: 2e-6 of the float64 gradient's largest magnitude.  The backward takes its signs from fp32 differences, so an element
with a contributing difference below 1e-6 in float64 may legitimately see another sign: those elements are left out, and their
share is asserted to be at most 0.1 %."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import SEED

pytestmark = pytest.mark.gpu

TILE = 32                      # csrc/grad_loss.hip: GL_TILE
# 1 x 1, single pairs, one-row and one-column maps, below the halo, ragged, multi-tile, the tile side -1 / exactly / +1 per dimension
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 2, 2), (1, 1, 40), (3, 27, 1), (3, 9, 17), (2, 16, 16), (2, 17, 33), (1, 64, 64),
          (2, 31, 70), (2, TILE - 1, TILE + 1), (1, TILE, TILE), (1, TILE + 1, TILE - 1), (1, 5, 7)]
CASES = [(shape, s) for shape in SHAPES for s in (1, 4)] + [(shape, s) for shape in ((1, 1, 2), (1, 2, 2)) for s in (2, 3)]
CASE_ID = lambda c: "x".join(map(str, c[0])) + f"-S{c[1]}"  # noqa: E731


# ------------------------------------------------------------------ the reference
def grad_loss_ref(a, b, scales):
    """The definition on (N, 3, H, W) tensors in their own dtype."""
    d = a - b
    total = d.new_zeros(())
    for s in range(scales):
        ds = d[..., ::2 ** s, ::2 ** s]
        if ds.shape[-1] > 1:
            total = total + (ds[..., :, 1:] - ds[..., :, :-1]).abs().mean()
        if ds.shape[-2] > 1:
            total = total + (ds[..., 1:, :] - ds[..., :-1, :]).abs().mean()
    return total / scales


def ref_value_and_grad(a, b, scales):
    x = a.to(torch.float64).clone().requires_grad_(True)
    loss = grad_loss_ref(x, b.to(torch.float64), scales)
    if not loss.requires_grad:                                  # a 1 x 1 image: no pair at all
        return float(loss), torch.zeros_like(x)
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g


def near_tie_mask(a, b, scales, eps=1e-6):
    """True where an element of the gradient has a contributing difference below eps in float64."""
    d = (a - b).to(torch.float64)
    mask = torch.zeros_like(d, dtype=torch.bool)
    for s in range(scales):
        ds, ms = d[..., ::2 ** s, ::2 ** s], mask[..., ::2 ** s, ::2 ** s]
        small = (ds[..., :, 1:] - ds[..., :, :-1]).abs() < eps
        ms[..., :, 1:] |= small
        ms[..., :, :-1] |= small
        small = (ds[..., 1:, :] - ds[..., :-1, :]).abs() < eps
        ms[..., 1:, :] |= small
        ms[..., :-1, :] |= small
    return mask


def run_op(pkg, a, b, scales, device, gout=None):
    """ops.grad_match_loss on fp32 copies of a, b -> (loss, d loss / d a on the CPU in float64, the loss tensor)."""
    x = a.to(torch.float32).to(device).requires_grad_(True)
    loss = pkg.ops.grad_match_loss(x, b.to(torch.float32).to(device), scales)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    if gout is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(gout, dtype=torch.float32, device=device))
    return float(loss.detach()), x.grad.detach().cpu().to(torch.float64), loss


def uniform_pair(shape, tag):
    """torch.rand values rounded to fp32 (the seeds of the structural-loss test): every evaluation sees the same numbers."""
    n, h, w = shape
    gen = torch.Generator().manual_seed(SEED + 97 * n + 13 * h + w + tag)
    return (torch.rand((n, 3, h, w), generator=gen, dtype=torch.float64).to(torch.float32).to(torch.float64),
            torch.rand((n, 3, h, w), generator=gen, dtype=torch.float64).to(torch.float32).to(torch.float64))


def grid_pair(shape, tag):
    """Values k / 4096, k < 4096: a - b and every difference of two such are exact in fp32."""
    n, h, w = shape
    gen = torch.Generator().manual_seed(SEED + 2000 + 97 * n + 13 * h + w + tag)
    return (torch.randint(0, 4096, (n, 3, h, w), generator=gen).to(torch.float64) / 4096.0,
            torch.randint(0, 4096, (n, 3, h, w), generator=gen).to(torch.float64) / 4096.0)


def assert_same_zeros_and_signs(g, gref):
    """Where the float64 gradient is zero (every sign term a tie or cancelled by its opposite; autograd may leave 1e-20 of its
    own summation order there) the kernel's is exactly zero; elsewhere the signs agree."""
    zero = gref.abs() <= 1e-9 * gref.abs().max()
    assert (g[zero] == 0).all()
    assert torch.equal(torch.sign(g[~zero]), torch.sign(gref[~zero]))


_REF = {}


def reference(kind, shape, scales):
    """(a, b, float64 loss, float64 gradient) of a case, computed once and shared; nobody writes to it."""
    key = (kind, shape, scales)
    if key not in _REF:
        a, b = (uniform_pair if kind == "uniform" else grid_pair)(shape, 0)
        _REF[key] = (a, b) + ref_value_and_grad(a, b, scales)
    return _REF[key]


# ------------------------------------------------------------------ 1. value and gradient
@pytest.mark.parametrize("case", CASES, ids=CASE_ID)
def test_loss_and_gradient_match_float64(case, pkg, device):
    shape, scales = case
    a, b, ref, gref = reference("uniform", shape, scales)
    loss, g, _ = run_op(pkg, a, b, scales, device)
    keep = ~near_tie_mask(a, b, scales)
    left_out = 1.0 - keep.double().mean().item()
    amax = gref.abs().max().item()
    err = ((g - gref).abs() * keep).max().item()
    print(f"{shape} S={scales}: loss {loss:.9f} ref {ref:.9f} rel {abs(loss - ref) / max(ref, 1e-6):.2e}; gradient max err {err:.2e} = "
          f"{err / max(amax, 1e-30):.2e} of amax {amax:.3e}; left out {left_out:.2%}")
    assert abs(loss - ref) <= 1e-6 * max(ref, 1e-6)
    assert left_out <= 1e-3
    assert torch.isfinite(g).all()
    assert err <= 2e-6 * amax
    if shape[1:] == (1, 1):
        assert loss == 0.0 and (g == 0).all()


# ------------------------------------------------------------------ 2. exact arithmetic
@pytest.mark.parametrize("case", CASES, ids=CASE_ID)
def test_grid_inputs_match_on_every_element(case, pkg, device):
    shape, scales = case
    a, b, ref, gref = reference("grid", shape, scales)
    loss, g, _ = run_op(pkg, a, b, scales, device)
    amax = gref.abs().max().item()
    err = (g - gref).abs().max().item()
    ulp = float(np.spacing(np.float32(ref)))
    print(f"{shape} S={scales}: loss {loss!r} ref {ref!r}: {abs(loss - ref) / ulp:.2f} ulp; gradient max err {err / max(amax, 1e-30):.2e} of amax")
    assert abs(loss - ref) <= 4 * ulp
    assert err <= 2e-6 * amax                                   # nothing left out
    assert_same_zeros_and_signs(g, gref)


@pytest.mark.parametrize("case", [((2, 17, 33), 4), ((1, 5, 7), 4), ((2, TILE + 1, 70), 3), ((1, 1, 2), 1)], ids=CASE_ID)
def test_a_constant_offset_is_all_ties(case, pkg, device):
    shape, scales = case
    _, b = grid_pair(shape, 1)
    loss, g, _ = run_op(pkg, b + 0.25, b, scales, device)
    assert loss == 0.0
    assert (g == 0).all()


@pytest.mark.parametrize("case", [((2, 17, 34), 1), ((2, 17, 34), 4), ((1, 40, 70), 4), ((1, TILE + 1, 2 * TILE), 3)], ids=CASE_ID)
def test_a_step_image_has_its_gradient_at_the_step(case, pkg, device):
    """The left half of `generated` lies 0.5 above the target, the right half on it: d is 0.5 | 0, every vertical pair is a tie and
    at scale s the one horizontal pair per selected row that straddles the step is not.  With one scale the gradient is non-zero
    in the two columns at the step only; with more, in the columns of the straddling pair of each scale, at rows and columns that
    scale selects.  Zeros and signs equal the float64 gradient's exactly, the values to the fp32 bound of the sign terms."""
    shape, scales = case
    n, h, w = shape
    _, b = grid_pair(shape, 2)
    c0 = w // 2                                                  # the first column of the right half
    a = b.clone()
    a[..., :c0] += 0.5
    ref, gref = ref_value_and_grad(a, b, scales)
    loss, g, _ = run_op(pkg, a, b, scales, device)
    allowed = torch.zeros((h, w), dtype=torch.bool)
    for s in range(scales):
        st = 2 ** s
        left = (c0 - 1) // st * st                               # the selected column at or left of the last offset column
        if left + st < w:
            allowed[::st, left] = True
            allowed[::st, left + st] = True
    if scales == 1:
        assert torch.equal(allowed.any(0).nonzero().flatten(), torch.tensor([c0 - 1, c0]))
    assert (g[:, :, ~allowed] == 0).all()
    assert (g != 0).any()
    assert_same_zeros_and_signs(g, gref)
    assert (g - gref).abs().max().item() <= 2e-6 * gref.abs().max().item()
    assert abs(loss - ref) <= 4 * float(np.spacing(np.float32(ref)))


# ------------------------------------------------------------------ 3. the physical buffers, through the C ABI
def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def abi_fwd(pkg, ap, bp, scales):
    lib = pkg._native.lib()
    n, h, w, _ = ap.shape
    need = lib.vcg_grad_loss_workspace(n, h, w, scales)
    assert need > 0
    ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=ap.device)
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=ap.device)
    rc = lib.vcg_grad_loss_fwd(_P(ap), _P(bp), _P(out), n, h, w, scales, _P(ws), need,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    pkg._native.check(rc, "vcg_grad_loss_fwd")
    return out.cpu()


def abi_bwd(pkg, ap, bp, scales, gout):
    """vcg_grad_loss_bwd with the gradient buffer poisoned beforehand -> (N, H, W, 4) on the CPU."""
    n, h, w, _ = ap.shape
    ga = torch.full_like(ap, float("nan"))
    g = torch.tensor([gout], dtype=torch.float32, device=ap.device)
    rc = pkg._native.lib().vcg_grad_loss_bwd(_P(ap), _P(bp), _P(g), _P(ga), n, h, w, scales,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    pkg._native.check(rc, "vcg_grad_loss_bwd")
    return ga.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", [((3, 9, 17), 1), ((2, 17, 33), 4), ((2, 31, 70), 4), ((1, 5, 7), 4), ((2, 1, 1), 4)], ids=CASE_ID)
def test_physical_buffers(case, pkg, device):
    shape, scales = case
    a, b, ref, gref = reference("uniform", shape, scales)
    ap = pkg.ops.as_phys(a.to(torch.float32).to(device)).clone()
    bp = pkg.ops.as_phys(b.to(torch.float32).to(device)).clone()
    out, ga = abi_fwd(pkg, ap, bp, scales), abi_bwd(pkg, ap, bp, scales, 1.0)
    # every pixel written, channel 3 exactly 0
    assert torch.isfinite(ga).all() and torch.isfinite(out).all()
    assert (ga[..., 3] == 0).all() and (_bits(ga[..., 3]) == 0).all()
    assert abs(float(out[0]) - ref) <= 1e-6 * max(ref, 1e-6)
    keep = ~near_tie_mask(a, b, scales)
    assert ((ga[..., :3].permute(0, 3, 1, 2).to(torch.float64) - gref).abs() * keep).max().item() <= 2e-6 * gref.abs().max().item()
    # channel 3 of the operands is never read into anything
    for fill in (float("nan"), 1e30):
        ap2, bp2 = ap.clone(), bp.clone()
        ap2[..., 3] = fill
        bp2[..., 3] = fill
        assert torch.equal(_bits(abi_fwd(pkg, ap2, bp2, scales)), _bits(out)), f"channel 3 = {fill} changed the loss"
        assert torch.equal(_bits(abi_bwd(pkg, ap2, bp2, scales, 1.0)), _bits(ga)), f"channel 3 = {fill} changed the gradient"
    # gout scales the gradient
    ga37 = abi_bwd(pkg, ap, bp, scales, 0.37)
    assert (ga37[..., 3] == 0).all() and torch.isfinite(ga37).all()
    assert (ga37.double() - 0.37 * ga.double()).abs().max().item() <= 1e-6 * 0.37 * ga.abs().max().item()
    # the same input gives the same bits
    assert torch.equal(_bits(abi_fwd(pkg, ap, bp, scales)), _bits(out))
    assert torch.equal(_bits(abi_bwd(pkg, ap, bp, scales, 1.0)), _bits(ga))


# ------------------------------------------------------------------ 4. ops.grad_match_loss
def test_op_refusals_and_result_type(pkg, device):
    a = torch.rand(2, 3, 9, 12, device=device)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        pkg.ops.grad_match_loss(a, torch.rand(2, 3, 9, 13, device=device))
    with pytest.raises(RuntimeError, match=r"\(N, 3, H, W\)"):
        pkg.ops.grad_match_loss(torch.rand(2, 4, 9, 12, device=device), torch.rand(2, 4, 9, 12, device=device))
    for bad in (0, 5, -1, 2.5):
        with pytest.raises(RuntimeError, match="scales"):
            pkg.ops.grad_match_loss(a, a.clone(), bad)
    with pytest.raises(RuntimeError, match="target"):
        pkg.ops.grad_match_loss(a, a.clone().requires_grad_(True))
    loss = pkg.ops.grad_match_loss(a, a.clone() * 0.5)          # scales defaults to 4
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    want = float(grad_loss_ref(a.cpu().double(), a.cpu().double() * 0.5, 4))
    assert abs(float(loss) - want) <= 1e-6 * want
    assert float(pkg.Losses.GradientMatchingLoss(2)(a, a.clone() * 0.5)) == float(pkg.ops.grad_match_loss(a, a.clone() * 0.5, 2))


def test_backward_without_a_gradient_to_compute_launches_nothing(pkg, device):
    """Only the (refused) target asks for a gradient: the function's backward runs and returns None for every input."""
    a = torch.rand(1, 3, 9, 12, device=device)
    b = torch.rand(1, 3, 9, 12, device=device).requires_grad_(True)
    loss = pkg.ops._ImageLossFn.apply(pkg.ops._GradTerm, a, b, 3)
    loss.backward()
    torch.cuda.synchronize()
    assert b.grad is None and a.grad is None


# ------------------------------------------------------------------ 5. the four models, two ranks: bodies shared with the other term
MODELS = ("autoencoder", "vae", "cycleaegan", "cyclevaegan")


@pytest.mark.parametrize("name", MODELS)
def test_models_add_and_report_the_term(name, pkg, device):
    from test_gpu_image_terms import models_add_and_report_the_term
    models_add_and_report_the_term("grad", name, pkg, device)


def test_other_architectures_are_refused_by_train_py(pkg):
    from test_gpu_image_terms import other_architectures_are_refused_by_train_py
    other_architectures_are_refused_by_train_py("grad", pkg)


def test_autoencoder_nan_guard_reports_the_term_as_nan(pkg, device):
    from test_gpu_image_terms import autoencoder_nan_guard_reports_the_term_as_nan
    autoencoder_nan_guard_reports_the_term_as_nan("grad", pkg, device)


def test_two_ranks_report_the_mean_and_stay_replicas(pkg, device, tmp_path):
    from test_gpu_image_terms import two_ranks_report_the_mean_and_stay_replicas
    two_ranks_report_the_mean_and_stay_replicas("grad", pkg, device, tmp_path)
