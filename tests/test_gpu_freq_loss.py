"""GPU: the focal frequency loss (csrc/freq_loss.hip, ops.freq_loss; lambda_freq / freq_alpha of the four models:
section 8, bodies in test_gpu_image_terms.py) against a float64 restatement of its definition on the CPU: torch.fft.fft2(..., norm="ortho") of generated - target, the weight
|D|^alpha over its plane maximum (0 where that maximum is 0, clamped to [0, 1], detached), the mean of w |D|^2, differentiated
by torch autograd.

Bounds.  The project's per-op parity bound, 1e-4 relative (README, "parity"): the loss against the float64 loss, every gradient
element against the largest magnitude of the float64 gradient.  The same definition evaluated in fp32 on the CPU sits at 1e-7 on
the loss and 4e-7 on the gradient, so the bound has room and still catches a wrong twiddle (one wrong table entry moves a whole
row or column of the spectrum by O(1 / sqrt(n))).  The errors measured on the GPU are in profiles/freq_loss_bench.txt.

The single-frequency plane: d = cos(2 pi (u y / H + v x / W)) has its whole spectrum in the two bins +-(u, v), each |D|^2 = H W / 4
with weight 1, so the loss is 0.5 and, by the definition's ga = 2 / (3 N H W) Re(F^H (w . D) F^H), the gradient is
2 d / (3 N H W) — the same as the Parseval case, whose weights are 1 everywhere.  (The issue that asked for this test wrote
d / (3 N H W) for it, which contradicts its own adjoint formula and float64 autograd; the test holds the formula.)"""
import ctypes
import math

import pytest
import torch

from conftest import SEED

pytestmark = pytest.mark.gpu

TOL = 1e-4
# degenerate axes; prime lengths; 3 N no tile multiple; one past / one short of MFMA tile edges; a multiple of 8 that is no power
# of two; more than one K chunk, ragged; the twiddle index wrapping many times
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 2, 3), (1, 3, 5), (3, 9, 17), (2, 16, 16), (2, 17, 33), (1, 31, 65), (1, 96, 40),
          (1, 130, 258), (1, 256, 256)]
ALPHAS = (0.0, 0.5, 1.0)
CASES = [(shape, alpha) for shape in SHAPES for alpha in ALPHAS]
CASE_ID = lambda c: "x".join(map(str, c[0])) + f"-a{c[1]}"  # noqa: E731


# ------------------------------------------------------------------ the reference
def freq_loss_ref(a, b, alpha):
    """The definition on (N, 3, H, W) tensors in their own dtype."""
    D = torch.fft.fft2(a - b, norm="ortho")
    p = D.real ** 2 + D.imag ** 2
    with torch.no_grad():
        m = torch.ones_like(p) if alpha == 0 else p ** (alpha / 2)
        top = m.amax(dim=(-2, -1), keepdim=True)
        w = torch.where(top > 0, m / torch.where(top > 0, top, torch.ones_like(top)), torch.zeros_like(m)).clamp(0.0, 1.0)
    return (w * p).mean()


def ref_value_and_grad(a, b, alpha):
    x = a.to(torch.float64).clone().requires_grad_(True)
    loss = freq_loss_ref(x, b.to(torch.float64), alpha)
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g


def run_op(pkg, a, b, alpha, device, gout=None):
    """ops.freq_loss on fp32 copies of a, b -> (loss, d loss / d a on the CPU in float64)."""
    x = a.to(torch.float32).to(device).requires_grad_(True)
    loss = pkg.ops.freq_loss(x, b.to(torch.float32).to(device), alpha)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    if gout is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(gout, dtype=torch.float32, device=device))
    return float(loss.detach()), x.grad.detach().cpu().to(torch.float64)


def uniform_pair(shape):
    """uniform(-1, 1) values rounded to fp32: every evaluation sees the same numbers."""
    n, h, w = shape
    gen = torch.Generator().manual_seed(SEED + 97 * n + 13 * h + w)
    draw = lambda: (torch.rand((n, 3, h, w), generator=gen, dtype=torch.float64) * 2 - 1).to(torch.float32).to(torch.float64)  # noqa: E731
    return draw(), draw()


_REF = {}


def reference(shape, alpha):
    """(a, b, float64 loss, float64 gradient) of a case, computed once and shared; nobody writes to it."""
    key = (shape, alpha)
    if key not in _REF:
        a, b = uniform_pair(shape)
        _REF[key] = (a, b) + ref_value_and_grad(a, b, alpha)
    return _REF[key]


# ------------------------------------------------------------------ 1. value and gradient
@pytest.mark.parametrize("case", CASES, ids=CASE_ID)
def test_loss_and_gradient_match_float64(case, pkg, device):
    shape, alpha = case
    a, b, ref, gref = reference(shape, alpha)
    loss, g = run_op(pkg, a, b, alpha, device)
    gmax = gref.abs().max().item()
    print(f"{CASE_ID(case)}: loss {loss:.8f} float64 {ref:.8f} rel {abs(loss - ref) / ref:.2e}; "
          f"gradient max err / max|g| {(g - gref).abs().max().item() / gmax:.2e}")
    assert abs(loss - ref) <= TOL * ref
    assert (g - gref).abs().max().item() <= TOL * gmax


# ------------------------------------------------------------------ 2. Parseval
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_alpha_zero_is_the_mean_square(shape, pkg, device):
    a, b = uniform_pair(shape)
    d = a - b
    loss, g = run_op(pkg, a, b, 0.0, device)
    want, gwant = (d * d).mean().item(), 2.0 * d / d.numel()
    assert abs(loss - want) <= TOL * want
    assert (g - gwant).abs().max().item() <= TOL * gwant.abs().max().item()


# ------------------------------------------------------------------ 3. one frequency
@pytest.mark.parametrize("case", [((2, 24, 40), 3, 7), ((1, 17, 33), 0, 5), ((1, 96, 40), 11, 0), ((1, 31, 65), 30, 64)],
                         ids=lambda c: str(c))
@pytest.mark.parametrize("alpha", ALPHAS)
def test_a_single_frequency_gives_one_half(case, alpha, pkg, device):
    (n, h, w), u, v = case
    y, x = torch.arange(h, dtype=torch.float64)[:, None], torch.arange(w, dtype=torch.float64)[None, :]
    d = torch.cos(2 * math.pi * (u * y / h + v * x / w)).expand(n, 3, h, w).contiguous()
    b = uniform_pair((n, h, w))[1]
    a = (b + d).to(torch.float32).to(torch.float64)                 # d as the fp32 operands really carry it
    d = a - b
    for gout in (None, -1.75):
        loss, g = run_op(pkg, a, b, alpha, device, gout)
        scale = 1.0 if gout is None else gout
        gwant = scale * 2.0 * d / d.numel()
        # the fp32 rounding of a = b + d leaves a noise floor of 1e-7 beside the two bins: within the bound
        assert abs(loss - 0.5) <= TOL * 0.5, loss
        assert (g - gwant).abs().max().item() <= TOL * gwant.abs().max().item()


# ------------------------------------------------------------------ 4. equal operands
@pytest.mark.parametrize("case", [((3, 9, 17), 1.0), ((2, 17, 33), 0.5), ((1, 96, 40), 0.0), ((1, 1, 1), 1.0)], ids=CASE_ID)
def test_equal_operands_give_exactly_zero(case, pkg, device):
    shape, alpha = case
    a, _ = uniform_pair(shape)
    loss, g = run_op(pkg, a, a.clone(), alpha, device)
    assert loss == 0.0 and not math.isnan(loss)
    assert (g == 0).all() and not torch.isnan(g).any()


# ------------------------------------------------------------------ 5. NaN
@pytest.mark.parametrize("case", [((3, 9, 17), 1.0), ((2, 17, 33), 0.0), ((1, 96, 40), 0.5), ((1, 1, 1), 1.0)], ids=CASE_ID)
def test_a_nan_operand_gives_a_nan_loss(case, pkg, device):
    shape, alpha = case
    a, b = uniform_pair(shape)
    a = a.clone()
    a[shape[0] - 1, 1, shape[1] // 2, shape[2] // 3] = float("nan")
    x = a.to(torch.float32).to(device)
    loss = pkg.ops.freq_loss(x, b.to(torch.float32).to(device), alpha)
    assert math.isnan(float(loss))


# ------------------------------------------------------------------ 6. the C entries on physical buffers
GUARD = 1024                       # floats after every buffer the library writes
SENTINEL = -7.25


def _guarded(nbytes, device):
    """A buffer of exactly nbytes (a multiple of 4) followed by a guard band; both filled with the sentinel."""
    assert nbytes % 4 == 0
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.float32, device=device)


def _guard_intact(t):
    return bool((t[-GUARD:] == SENTINEL).all())


def abi_run(pkg, ap, bp, alpha, gout):
    """vcg_freq_loss_fwd then _bwd with out, spec, ws and ga at exactly the sizes the library asks for, each followed by a guard
    band -> (out (1,), ga (N, H, W, 4)) on the CPU."""
    lib, P = pkg._native.lib(), ctypes.c_void_p
    n, h, w, _ = ap.shape
    dev = ap.device
    need, keep = lib.vcg_freq_loss_workspace(n, h, w), lib.vcg_freq_loss_spectrum(n, h, w)
    assert need and keep
    out, spec, ws, ws2 = _guarded(4, dev), _guarded(keep, dev), _guarded(need, dev), _guarded(need, dev)
    ga = _guarded(n * h * w * 16, dev)
    g = torch.tensor([gout], dtype=torch.float32, device=dev)       # read from device memory
    st = P(torch.cuda.current_stream().cuda_stream)
    rc = lib.vcg_freq_loss_fwd(P(ap.data_ptr()), P(bp.data_ptr()), P(out.data_ptr()), n, h, w, alpha, P(spec.data_ptr()), keep,
                               P(ws.data_ptr()), need, st)
    pkg._native.check(rc, "vcg_freq_loss_fwd")
    rc = lib.vcg_freq_loss_bwd(P(spec.data_ptr()), keep, P(g.data_ptr()), P(ga.data_ptr()), n, h, w, alpha, P(ws2.data_ptr()),
                               need, st)
    pkg._native.check(rc, "vcg_freq_loss_bwd")
    torch.cuda.synchronize()
    for name, t in (("out", out), ("spec", spec), ("ws", ws), ("ws (backward)", ws2), ("ga", ga)):
        assert _guard_intact(t), f"the guard band after {name} was written"
    body = ga[:-GUARD]
    assert not (body == SENTINEL).any(), "a pixel of ga was not written"
    return out[:1].cpu(), body.view(n, h, w, 4).cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", [((3, 9, 17), 1.0), ((2, 17, 33), 0.5), ((1, 31, 65), 1.0), ((1, 130, 258), 1.0), ((2, 1, 1), 0.0)],
                         ids=CASE_ID)
def test_physical_buffers(case, pkg, device):
    shape, alpha = case
    a, b, ref, gref = reference(shape, alpha)
    ap = pkg.ops.as_phys(a.to(torch.float32).to(device)).clone()
    bp = pkg.ops.as_phys(b.to(torch.float32).to(device)).clone()
    out, ga = abi_run(pkg, ap, bp, alpha, 1.0)
    assert torch.isfinite(ga).all() and torch.isfinite(out).all()
    assert (ga[..., 3] == 0).all()
    assert abs(float(out[0]) - ref) <= TOL * ref
    assert (ga[..., :3].permute(0, 3, 1, 2).to(torch.float64) - gref).abs().max().item() <= TOL * gref.abs().max().item()
    # channel 3 of the operands is never read
    ap2, bp2 = ap.clone(), bp.clone()
    ap2[..., 3] = float("nan")
    bp2[..., 3] = float("nan")
    out2, ga2 = abi_run(pkg, ap2, bp2, alpha, 1.0)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(ga2), _bits(ga)), "channel 3 = NaN changed the result"
    # gout is read on the device and scales the gradient
    out37, ga37 = abi_run(pkg, ap, bp, alpha, 0.37)
    assert torch.equal(_bits(out37), _bits(out))
    assert (ga37[..., 3] == 0).all()
    assert (ga37.double() - 0.37 * ga.double()).abs().max().item() <= 1e-6 * 0.37 * ga.abs().max().item()
    # the same input gives the same bits
    out3, ga3 = abi_run(pkg, ap, bp, alpha, 1.0)
    assert torch.equal(_bits(out3), _bits(out)) and torch.equal(_bits(ga3), _bits(ga))


# ------------------------------------------------------------------ 7. ops.freq_loss
def test_op_refusals_and_result_type(pkg, device):
    a = torch.rand(2, 3, 9, 12, device=device)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.ops.freq_loss(torch.rand(2, 3, 9, 12), torch.rand(2, 3, 9, 12))
    with pytest.raises(RuntimeError, match="shape mismatch"):
        pkg.ops.freq_loss(a, torch.rand(2, 3, 9, 13, device=device))
    with pytest.raises(RuntimeError, match=r"\(N, 3, H, W\)"):
        pkg.ops.freq_loss(torch.rand(2, 4, 9, 12, device=device), torch.rand(2, 4, 9, 12, device=device))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="alpha"):
            pkg.ops.freq_loss(a, a.clone(), bad)
    with pytest.raises(RuntimeError, match="target"):
        pkg.ops.freq_loss(a, a.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="cap"):
        pkg.ops.freq_loss(torch.zeros(1, 3, 1, 2049, device=device), torch.zeros(1, 3, 1, 2049, device=device))
    loss = pkg.ops.freq_loss(a, a.clone() * 0.5)                 # alpha defaults to 1
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    want = float(freq_loss_ref(a.cpu().double(), a.cpu().double() * 0.5, 1.0))
    assert abs(float(loss) - want) <= TOL * want
    assert float(pkg.Losses.FocalFrequencyLoss(0.5)(a, a.clone() * 0.5)) == float(pkg.ops.freq_loss(a, a.clone() * 0.5, 0.5))


def test_backward_without_a_gradient_to_compute_launches_nothing(pkg, device, monkeypatch):
    """Only the (refused) target asks for a gradient: the function's backward runs, returns None for every input and never
    reaches the library's backward entry."""
    a = torch.rand(1, 3, 9, 12, device=device)
    b = torch.rand(1, 3, 9, 12, device=device).requires_grad_(True)
    loss = pkg.ops._ImageLossFn.apply(pkg.ops._FreqTerm, a, b, 1.0)
    called = []
    lib = pkg._native.lib()
    real = lib.vcg_freq_loss_bwd
    monkeypatch.setattr(lib, "vcg_freq_loss_bwd", lambda *args: called.append(1) or real(*args))
    loss.backward()
    torch.cuda.synchronize()
    assert b.grad is None and a.grad is None and not called


# ------------------------------------------------------------------ 8. the four models, two ranks: bodies shared with the other term
MODELS = ("autoencoder", "vae", "cycleaegan", "cyclevaegan")


@pytest.mark.parametrize("name", MODELS)
def test_models_add_and_report_the_term(name, pkg, device):
    from test_gpu_image_terms import models_add_and_report_the_term
    models_add_and_report_the_term("freq", name, pkg, device)


def test_other_architectures_are_refused_by_train_py(pkg):
    from test_gpu_image_terms import other_architectures_are_refused_by_train_py
    other_architectures_are_refused_by_train_py("freq", pkg)


def test_autoencoder_nan_guard_reports_the_term_as_nan(pkg, device):
    from test_gpu_image_terms import autoencoder_nan_guard_reports_the_term_as_nan
    autoencoder_nan_guard_reports_the_term_as_nan("freq", pkg, device)


def test_two_ranks_report_the_mean_and_stay_replicas(pkg, device, tmp_path):
    from test_gpu_image_terms import two_ranks_report_the_mean_and_stay_replicas
    two_ranks_report_the_mean_and_stay_replicas("freq", pkg, device, tmp_path)
