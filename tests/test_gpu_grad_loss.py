"""GPU: the multi-scale gradient-matching loss (csrc/grad_loss.hip, ops.grad_match_loss, lambda_grad / grad_scales of the four
models) against a float64 torch restatement of its definition, differentiated by torch autograd on the CPU: strided slicing,
`.abs().mean()` per direction and scale, a direction without a pair contributing 0, the sum divided by the number of scales.

Bounds.  The kernel forms d = a - b and the pair differences in double (exact for fp32 inputs) and sums in double, so the loss
carries the two conversions to fp32 only: 1e-6 relative.  A gradient element is a sum of at most 16 sign terms, each rounded once
in fp32: 2e-6 of the float64 gradient's largest magnitude.  The backward takes its signs from fp32 differences, so an element
with a contributing difference below 1e-6 in float64 may legitimately see another sign: those elements are left out, and their
share is asserted to be at most 0.1 %."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import SEED

pytestmark = pytest.mark.gpu

TILE = 32                      # csrc/grad_loss.hip: GL_TILE
LR = 2e-4
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
    loss = pkg.ops._GradLossFn.apply(a, b, 3)
    loss.backward()
    torch.cuda.synchronize()
    assert b.grad is None and a.grad is None


# ------------------------------------------------------------------ 5. the four models
LAMBDA, SCALES = 0.5, 3
MODELS = ("autoencoder", "vae", "cycleaegan", "cyclevaegan")
# G_loss as the weighted sum of the reported terms (configure_loss's defaults; the cycle models unpaired)
WEIGHTS = {"autoencoder": {"loss_trans": 1.0}, "vae": {"loss_trans": 1.0, "loss_kl": 1e-5},
           "cycleaegan": {"loss_cycle": 10.0, "loss_gan_g": 1.0}, "cyclevaegan": {"loss_cycle": 10.0, "loss_gan_g": 1.0, "loss_kl": 1e-5}}


def _make(pkg, name):
    N = pkg.Networks
    return {"autoencoder": N.Autoencoder, "vae": lambda: N.VariationalAutoencoder(latent_dim=64),
            "cycleaegan": lambda: N.CycleAEGAN(paired=False), "cyclevaegan": lambda: N.CycleVAEGAN(latent_dim=64, paired=False)}[name]()


def _model_batch(pkg, name, device):
    """batch 2; 32 x 32 for the two single generators, 256 x 256 for the cycle models (their discriminators admit nothing less)"""
    x, y = pkg.synth.batch(2, 32 if name in ("autoencoder", "vae") else 256, SEED)
    return {"x": torch.from_numpy(x).to(device), "y": torch.from_numpy(y).to(device)}


def _twins(pkg, device, name, count):
    """`count` models with equal weights, optimizers configured, losses not yet."""
    torch.manual_seed(SEED)
    first = _make(pkg, name)
    sd = {k: v.clone() for k, v in first.state_dict().items()}
    out = []
    for i in range(count):
        m = first if i == 0 else _make(pkg, name)
        m.load_state_dict(sd)
        m = m.to(device).train()
        m.configure_optimizers(lr=LR)
        out.append(m)
    return out, sd


def _flat_params(m):
    return [getattr(m, n).flat_param for n in m._opt_names]


def _same_bits(ma, mb):
    assert list(ma) == list(mb), f"metric keys {list(ma)} vs {list(mb)}"
    for k in ma:
        assert np.float64(ma[k]).tobytes() == np.float64(mb[k]).tobytes(), f"{k}: {ma[k]!r} vs {mb[k]!r}"


def _operands(pkg, name, model, batch):
    """The (generated, target) pairs the step's gradient-matching term sees, from `model`'s own forward, on the CPU in float64."""
    c = lambda t: t.detach().cpu().to(torch.float64)  # noqa: E731
    with torch.no_grad():
        if name == "autoencoder":
            return [(c(model(pkg.ops.to_nhwc(batch["x"]))), c(batch["y"]))]
        if name == "vae":
            return [(c(model(pkg.ops.to_nhwc(batch["x"]))[0]), c(batch["y"]))]
        outs = model(batch["x"], batch["y"])                     # Gx, FGx, Fy, GFy, ...
        return [(c(outs[1]), c(batch["x"])), (c(outs[3]), c(batch["y"]))]


@pytest.mark.parametrize("name", MODELS)
def test_models_add_and_report_the_term(name, pkg, device):
    (on, twin, plain), sd = _twins(pkg, device, name, 3)
    batch = _model_batch(pkg, name, device)
    kw = dict(lambda_grad=LAMBDA, grad_scales=SCALES)
    on.configure_loss(**kw)
    twin.configure_loss(lambda_ssim=0.25, **kw)
    plain.configure_loss()
    # the operands, and the key order with both optional terms on, from the twin; then the twin gets its weights (and the power
    # iteration's u, v, which its forwards advanced) back and becomes the lambda_grad = 0 model
    pkg.ops.manual_seed(SEED)
    pairs = _operands(pkg, name, twin, batch)
    want = sum(float(grad_loss_ref(g, t, SCALES)) for g, t in pairs)
    pkg.ops.manual_seed(SEED)
    v_both = twin.validation_step(batch)
    keys = [k for k in v_both if k not in ("Gx", "Fy")]
    assert keys[-2:] == ["loss_ssim", "loss_grad"], keys
    twin.load_state_dict(sd)
    twin.configure_loss(lambda_grad=0.0, grad_scales=SCALES)

    pkg.ops.manual_seed(SEED)
    v_on = on.validation_step(batch)
    pkg.ops.manual_seed(SEED)
    m_on = on.training_step(batch)
    pkg.ops.manual_seed(SEED)
    m_zero = twin.training_step(batch)
    pkg.ops.manual_seed(SEED)
    m_plain = plain.training_step(batch)

    for what, m in (("training_step", m_on), ("validation_step", v_on)):
        got = m["loss_grad"]
        print(f"{name} {what}: loss_grad {got:.8f} float64 {want:.8f} rel {abs(got - want) / want:.2e}; G_loss {m['G_loss']:.7f}")
        assert abs(got - want) <= 1e-5 * want
        expect = sum(w * m[k] for k, w in WEIGHTS[name].items()) + LAMBDA * m["loss_grad"]
        assert abs(m["G_loss"] - expect) <= 1e-6 * abs(expect), f"{name} {what}: G_loss {m['G_loss']!r}, weighted sum {expect!r}"
    assert [k for k in m_on if k not in m_plain] == ["loss_grad"] and list(m_on)[:len(m_plain)] == list(m_plain)
    assert "loss_grad" not in m_zero
    # off is off: the weight 0 and the missing keyword take the same step, bit for bit
    _same_bits(m_zero, m_plain)
    for pa, pb, pc in zip(_flat_params(twin), _flat_params(plain), _flat_params(on)):
        assert torch.equal(_bits(pa), _bits(pb))
    assert not torch.equal(_flat_params(on)[0], _flat_params(plain)[0])


def test_other_architectures_are_refused_by_train_py(pkg):
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")
    args = train.build_parser().parse_args(["--architecture", "cyclevae", "--lambda_grad", "0.5"])
    with pytest.raises(ValueError, match="lambda_grad") as e:
        train.main(args)
    assert all(name in str(e.value) for name in MODELS)


def test_autoencoder_nan_guard_reports_the_term_as_nan(pkg, device):
    (m,), _ = _twins(pkg, device, "autoencoder", 1)
    m.configure_loss(lambda_ssim=0.25, lambda_grad=LAMBDA, grad_scales=SCALES)
    batch = _model_batch(pkg, "autoencoder", device)
    bad = batch["x"].clone()
    bad[0, 1, 5, 7] = float("nan")
    got = m.training_step({"x": bad, "y": batch["y"]})
    assert got["nan_detected"] is True
    assert list(got)[-2:] == ["loss_ssim", "loss_grad"] and got["loss_grad"] != got["loss_grad"] and got["loss_ssim"] != got["loss_ssim"]


# ------------------------------------------------------------------ 6. two ranks
def test_two_ranks_report_the_mean_and_stay_replicas(pkg, device, tmp_path):
    """test_gpu_dp_options.py's worker, unchanged: two `spawn` ranks with a batch of 1 each on the one card (4 hardware queues
    each), joined under its limit, nothing started after a failure.  One CycleVAEGAN step with the term on."""
    import shutil

    import test_gpu_dp_options as dp
    arch, step = "cyclevaegan", dp.STEPS[0]
    loss_kw = dict(lambda_grad=LAMBDA, grad_scales=SCALES)
    cfg = dp._cfg(arch, tmp_path, tag="grad", loss_kw=loss_kw, buffers=("flat_param",), steps=(step,))
    try:
        dp._run_two_ranks(cfg)
        recs = [dp._load(cfg, r, "step0") for r in range(2)]
        dp._assert_replicas(recs[0], recs[1], dp._opt_names(arch), "gradient-matching step")
        for name in dp._opt_names(arch):
            assert recs[0][f"{name}.flat_param"] is not None
        # each rank's shard alone, in this process: the same weights, images and eps; a validation step leaves the weights alone
        model = dp._configured(pkg, arch, device, dp.LR, {}, loss_kw)
        alone = []
        for r in range(2):
            dp._inject_eps(pkg, arch, step, slice(r, r + 1))
            alone.append(model.validation_step(dp._batch(pkg, arch, step, device, slice(r, r + 1)))["loss_grad"])
        mean = 0.5 * (alone[0] + alone[1])
        for r, rec in enumerate(recs):
            got = rec["metrics"]["loss_grad"]
            print(f"rank {r}: loss_grad {got!r}; shards alone {alone}, mean {mean!r}")
            assert abs(got - mean) <= 1e-6 * mean
        assert recs[0]["metrics"]["loss_grad"] == recs[1]["metrics"]["loss_grad"]
        assert abs(alone[0] - alone[1]) > 1e-4 * mean            # the shards differ: a rank's own value is not the mean
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
