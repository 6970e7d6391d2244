"""GPU: the structural loss (csrc/ssim_loss.hip, ops.ssim_loss, lambda_ssim of the four models) against a float64 torch
restatement of its formula, differentiated by torch autograd on the CPU: a grouped conv2d with the outer product of the normalised
Gaussian, sigma = E[.^2] - mu^2.  The same function evaluated in float32 is the yardstick of the cancellation cases."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import SEED, assert_grad_checksum, checksum, in_cancelled_bias

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from cases import LR, STEP_BIAS_STD  # noqa: E402

pytestmark = pytest.mark.gpu

# one window position, one-row and one-column maps, a tile side +-1, ragged multi-tile maps, N not a power of two
SHAPES = [(1, 11, 11), (1, 11, 40), (3, 27, 12), (2, 16, 16), (2, 17, 17), (1, 26, 27), (2, 33, 48), (1, 64, 64)]


# ------------------------------------------------------------------ the reference
def window(dtype):
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-d * d / (2.0 * 1.5 * 1.5))
    return (g / g.sum()).to(dtype)


def ssim_loss_ref(a, b):
    """1 - mean SSIM of (N, 3, H, W) tensors in their own dtype."""
    w = window(a.dtype)
    k = torch.outer(w, w)[None, None].repeat(3, 1, 1, 1)
    mu_a, mu_b = F.conv2d(a, k, groups=3), F.conv2d(b, k, groups=3)
    s_a = F.conv2d(a * a, k, groups=3) - mu_a * mu_a
    s_b = F.conv2d(b * b, k, groups=3) - mu_b * mu_b
    s_ab = F.conv2d(a * b, k, groups=3) - mu_a * mu_b
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * mu_a * mu_b + c1) * (2 * s_ab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (s_a + s_b + c2))
    return 1 - s.mean()


def ref_value_and_grad(a, b, dtype):
    x = a.to(dtype).clone().requires_grad_(True)
    loss = ssim_loss_ref(x, b.to(dtype))
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g.to(torch.float64)


def run_op(pkg, a, b, device, gout=None):
    """ops.ssim_loss on fp32 copies of a, b -> (loss, d loss / d a on the CPU in float64, the loss tensor)."""
    x = a.to(torch.float32).to(device).requires_grad_(True)
    loss = pkg.ops.ssim_loss(x, b.to(torch.float32).to(device))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    if gout is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(gout, dtype=torch.float32, device=device))
    return float(loss.detach()), x.grad.detach().cpu().to(torch.float64), loss


def abi_bwd(pkg, a, b, device, gout):
    """vcg_ssim_loss_bwd on physical buffers, the gradient buffer poisoned beforehand -> (N, H, W, 4) on the CPU."""
    ap = pkg.ops.as_phys(a.to(torch.float32).to(device))
    bp = pkg.ops.as_phys(b.to(torch.float32).to(device))
    n, h, w, _ = ap.shape
    ga = torch.full_like(ap, float("nan"))
    g = torch.tensor([gout], dtype=torch.float32, device=device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = pkg._native.lib().vcg_ssim_loss_bwd(P(ap), P(bp), P(g), P(ga), n, h, w,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    pkg._native.check(rc, "vcg_ssim_loss_bwd")
    return ga.cpu()


def uniform_pair(shape, tag):
    n, h, w = shape
    gen = torch.Generator().manual_seed(SEED + 97 * n + 13 * h + w + tag)
    return (torch.rand((n, 3, h, w), generator=gen, dtype=torch.float64).to(torch.float32).to(torch.float64),
            torch.rand((n, 3, h, w), generator=gen, dtype=torch.float64).to(torch.float32).to(torch.float64))


# ------------------------------------------------------------------ 1. value and gradient
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_match_float64(shape, pkg, device):
    a, b = uniform_pair(shape, 0)
    ref, gref = ref_value_and_grad(a, b, torch.float64)
    loss, g, _ = run_op(pkg, a, b, device)
    amax = gref.abs().max().item()
    err = (g - gref).abs().max().item()
    print(f"{shape}: loss {loss:.8f} ref {ref:.8f} |d| {abs(loss - ref):.2e}; gradient max err {err:.2e} = {err / amax:.2e} of amax")
    assert abs(loss - ref) <= 1e-5
    assert err <= 1e-4 * amax
    # the physical buffer: every pixel written, channel 3 exactly 0, nothing non-finite
    phys = abi_bwd(pkg, a, b, device, 1.0)
    assert torch.isfinite(phys).all()
    assert (phys[..., 3] == 0).all()
    assert torch.equal(phys[..., :3].permute(0, 3, 1, 2).to(torch.float64), g)
    # gout scales the gradient
    _, g37, _ = run_op(pkg, a, b, device, gout=0.37)
    assert (g37 - 0.37 * g).abs().max().item() <= 1e-6 * 0.37 * g.abs().max().item()
    phys37 = abi_bwd(pkg, a, b, device, 0.37)
    assert (phys37[..., 3] == 0).all() and torch.isfinite(phys37).all()


# ------------------------------------------------------------------ 2. where the moments cancel
def cancelling_pair(shape, kind):
    n, h, w = shape
    gen = torch.Generator().manual_seed(SEED + 1000 + 97 * n + 13 * h + w)
    if kind == "ramp":
        y = torch.linspace(0, 1, h, dtype=torch.float64)[:, None]
        x = torch.linspace(0, 1, w, dtype=torch.float64)[None, :]
        b = (0.2 + 0.3 * (y + x)).expand(n, 3, h, w).contiguous()
        a = b + 0.01 * torch.randn((n, 3, h, w), generator=gen, dtype=torch.float64)
    else:
        b = torch.full((n, 3, h, w), 0.5, dtype=torch.float64)
        a = b + 1e-3 * torch.randn((n, 3, h, w), generator=gen, dtype=torch.float64)
    # the inputs ARE fp32 numbers: all three evaluations see the same values
    return a.to(torch.float32).to(torch.float64), b.to(torch.float32).to(torch.float64)


@pytest.mark.parametrize("kind", ["ramp", "flat"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_worse_than_float32_torch_where_moments_cancel(shape, kind, pkg, device):
    """Figures (MI355X; error against float64 of this kernel | of the float32 torch evaluation of the same formula):
    see DESIGN.md, "The structural loss", which holds the table this test prints."""
    a, b = cancelling_pair(shape, kind)
    ref, gref = ref_value_and_grad(a, b, torch.float64)
    l32, g32 = ref_value_and_grad(a, b, torch.float32)
    loss, g, _ = run_op(pkg, a, b, device)
    amax = gref.abs().max().item()
    e_hip, e_f32 = (g - gref).abs().max().item(), (g32 - gref).abs().max().item()
    print(f"SSIMTABLE {kind:5s} {str(shape):12s} loss err hip {abs(loss - ref):.2e} f32 {abs(l32 - ref):.2e} | "
          f"grad err / amax hip {e_hip / amax:.2e} f32 {e_f32 / amax:.2e}")
    assert torch.isfinite(g).all()
    assert abs(loss - ref) <= abs(l32 - ref)
    assert e_hip <= e_f32


# ------------------------------------------------------------------ 3. a = b
@pytest.mark.parametrize("shape", [(1, 11, 11), (2, 17, 17), (2, 33, 48)], ids=lambda s: "x".join(map(str, s)))
def test_identical_images_give_zero_loss_and_a_finite_gradient(shape, pkg, device):
    a, _ = uniform_pair(shape, 1)
    loss, g, _ = run_op(pkg, a, a.clone(), device)
    assert abs(loss) <= 1e-6
    assert torch.isfinite(g).all()


# ------------------------------------------------------------------ 4. determinism, batch independence
def test_two_calls_return_the_same_bits_and_an_image_does_not_see_its_batch(pkg, device):
    a, b = uniform_pair((3, 33, 48), 2)
    l1, g1, t1 = run_op(pkg, a, b, device)
    l2, g2, t2 = run_op(pkg, a, b, device)
    assert torch.equal(t1, t2) and torch.equal(g1, g2)
    _, g_alone, _ = run_op(pkg, a[:1], b[:1], device)
    assert (3.0 * g1[:1] - g_alone).abs().max().item() <= 1e-6 * g_alone.abs().max().item()


# ------------------------------------------------------------------ 5. refusals
def test_small_images_and_differentiable_targets_are_refused(pkg, device):
    a = torch.rand(1, 3, 10, 16, device=device)
    with pytest.raises(RuntimeError, match="11x11 window"):
        pkg.ops.ssim_loss(a, a.clone())
    a = torch.rand(1, 3, 16, 10, device=device)
    with pytest.raises(RuntimeError, match="11x11 window"):
        pkg.ops.ssim_loss(a, a.clone())
    a = torch.rand(1, 3, 16, 16, device=device)
    with pytest.raises(RuntimeError, match="target"):
        pkg.ops.ssim_loss(a, a.clone().requires_grad_(True))


# ------------------------------------------------------------------ 6. autoencoder / VAE steps end to end
def _synth_model(pkg, model, key):
    from test_gpu_parity import load_synth
    return load_synth(pkg, model, key, STEP_BIAS_STD)


def _check_step(pkg, device, model, P, got, forward, key):
    """got: the step's metrics; forward(Q, dtype) -> dict of the oracle's loss tensors with "G_loss" among them.  Metrics to the
    1e-3 the step tests of tests/test_gpu_parity.py hold them to, every parameter gradient by `assert_grad_checksum`
    (error against the float64 gradient within 4 x the float32 oracle's own, or the ReLU-flip budget)."""
    res = {}
    for dtype in (torch.float64, torch.float32):
        Q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()}
        t = forward(Q, dtype)
        names = list(Q)
        gs = torch.autograd.grad(t["G_loss"], [Q[n] for n in names], allow_unused=True)
        res[dtype] = ({k: float(v.detach()) for k, v in t.items()}, dict(zip(names, gs)))
    want, g64 = res[torch.float64]
    _, g32 = res[torch.float32]
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-3 * max(abs(v), 1e-6), f"{key}: {k} = {got[k]!r}, float64 oracle {v!r}"
    bad = []
    for n, p in model.named_parameters():
        if in_cancelled_bias(n) or g64[n] is None:
            continue
        try:
            assert_grad_checksum(p.grad, checksum(g32[n].to(device)), checksum(g64[n].to(device)), "grad " + n, key=key)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, f"{len(bad)} gradients off:\n" + "\n".join(b[:300] for b in bad[:8])


def _target_clear_of_l1_kinks(x, out64, out32):
    """The step's target: the input image x, moved where it lies within rounding of the network's output.

    d|out - y| / d out = sign(out - y) is a step function, so a gradient comparison with a tolerance means something only where no
    element of out - y is within the forward's own float32 error of zero: one flipped sign moves d loss / d out by 2 / n of an
    element, sqrt(4 / n) of its norm.  The flip budget of the step tests (conftest.FLIP_BUDGET, 1e-2) is calibrated on one flip
    among 65 536 activations; at this test's 32 x 32, batch 2, the output has n = 6 144 elements and ONE flip is 2.6e-2 of the
    norm, above the budget by itself.  With y = x and these weights the float64 output comes within 2.5e-4 of x, the float32
    oracle's output is 3.5e-3 off the float64 one (the 2 x 2 bottleneck maps have near-dead channels whose InstanceNorm
    amplifies rounding 300-fold), and the device step measured two flipped signs where the float32 oracle happened to have
    none: decoder.model.5.conv.bias (= sum of signs / n) 1.9e-2 off, its weight 6.2e-2, the encoder weights 2.5e-1 .. 5.3e-1,
    with lambda_ssim = 0 as with 0.5.  So the target keeps clear of the kinks by a margin taken from the reference's own error:
    tau = 4 x max |out32 - out64| (the 4 x of assert_grad_checksum); where |out64 - x| < tau, y is out64 -+ tau (a few elements
    of 6 144, moved by less than 2 tau); elsewhere y = x.  Nothing here looks at the device's output."""
    x64 = x.to(torch.float64)
    tau = 4.0 * (out32.to(torch.float64) - out64).abs().max().item()
    d = out64 - x64
    side = torch.where(d >= 0, torch.ones_like(d), -torch.ones_like(d))
    y = torch.where(d.abs() < tau, out64 - 2.0 * tau * side, x64).to(torch.float32)
    assert ((out64 - y.to(torch.float64)).abs() >= tau).all()
    return y, int((d.abs() < tau).sum()), tau


def test_autoencoder_step_with_the_structural_term_matches_the_oracle(pkg, oracle, device):
    key = "ae32ssim"
    model = pkg.Networks.Autoencoder()
    P = _synth_model(pkg, model, key)
    model = model.to(device).train()
    model.configure_optimizers(lr=LR)
    model.configure_loss(lambda_ssim=0.5)
    x, _ = pkg.synth.batch(2, 32, SEED)
    xb = torch.from_numpy(x)
    with torch.no_grad():
        o64 = oracle.autoencoder_forward(xb.to(torch.float64), {k: v.to(torch.float64) for k, v in P.items()})
        o32 = oracle.autoencoder_forward(xb, P)
    yb, moved, tau = _target_clear_of_l1_kinks(xb, o64, o32)
    print(f"{key}: tau {tau:.2e}, {moved} of {xb.numel()} target elements moved")
    assert moved <= xb.numel() // 100
    got = model.training_step({"x": xb.to(device), "y": yb.to(device)})
    assert list(got) == ["G_loss", "loss_trans", "total_loss", "loss_ssim"]
    assert got["total_loss"] == got["G_loss"]

    def forward(Q, dtype):
        out = oracle.autoencoder_forward(xb.to(dtype), Q)
        lt, ls = oracle.l1(out, yb.to(dtype)), ssim_loss_ref(out, yb.to(dtype))
        return {"loss_trans": lt, "loss_ssim": ls, "G_loss": lt + 0.5 * ls}
    _check_step(pkg, device, model, P, got, forward, key)
    with torch.no_grad():
        v = model.validation_step({"x": xb.to(device), "y": yb.to(device)})
    assert set(v) == {"G_loss", "total_loss", "loss_trans", "loss_ssim", "Gx"}
    assert abs(v["G_loss"] - (v["loss_trans"] + 0.5 * v["loss_ssim"])) <= 1e-5


def test_vae_step_with_the_structural_term_matches_the_oracle(pkg, oracle, device):
    key = "vae32ssim"
    model = pkg.Networks.VariationalAutoencoder(latent_dim=64)
    P = _synth_model(pkg, model, key)
    model = model.to(device).train()
    model.configure_optimizers(lr=LR)
    model.configure_loss(lambda_kl=1e-5, lambda_ssim=0.5)
    x, _ = pkg.synth.batch(2, 32, SEED)
    xb = torch.from_numpy(x)
    eps = torch.from_numpy(pkg.synth.eps_list(1, (2, 64, 2, 2), SEED)[0])
    with torch.no_grad():
        o64 = oracle.vae_forward(xb.to(torch.float64), {k: v.to(torch.float64) for k, v in P.items()}, "", eps.to(torch.float64))[0]
        o32 = oracle.vae_forward(xb, P, "", eps)[0]
    yb, moved, tau = _target_clear_of_l1_kinks(xb, o64, o32)
    print(f"{key}: tau {tau:.2e}, {moved} of {xb.numel()} target elements moved")
    assert moved <= xb.numel() // 100
    pkg.ops.inject_eps([eps])
    got = model.training_step({"x": xb.to(device), "y": yb.to(device)})
    assert list(got) == ["G_loss", "loss_trans", "loss_kl", "loss_ssim"]

    def forward(Q, dtype):
        out, mu, lv = oracle.vae_forward(xb.to(dtype), Q, "", eps.to(dtype))
        lt, lk, ls = oracle.l1(out, yb.to(dtype)), oracle.kl_loss(mu, lv), ssim_loss_ref(out, yb.to(dtype))
        return {"loss_trans": lt, "loss_kl": lk, "loss_ssim": ls, "G_loss": lt + 1e-5 * lk + 0.5 * ls}
    _check_step(pkg, device, model, P, got, forward, key)
    pkg.ops.inject_eps([eps])
    v = model.validation_step({"x": xb.to(device), "y": yb.to(device)})
    assert set(v) == {"G_loss", "loss_trans", "loss_kl", "loss_ssim", "Gx"}


# ------------------------------------------------------------------ 7. the off switch
def _twins(pkg, device, make, configure):
    """Two models with equal weights, one per `configure` entry."""
    torch.manual_seed(SEED)
    first = make()
    sd = {k: v.clone() for k, v in first.state_dict().items()}
    out = []
    for i, kw in enumerate(configure):
        m = first if i == 0 else make()
        m.load_state_dict(sd)
        m = m.to(device).train()
        m.configure_optimizers(lr=LR)
        m.configure_loss(**kw)
        out.append(m)
    return out


def _same_bits(ma, mb):
    assert list(ma) == list(mb), f"metric keys {list(ma)} vs {list(mb)}"
    for k in ma:
        assert np.float64(ma[k]).tobytes() == np.float64(mb[k]).tobytes(), f"{k}: {ma[k]!r} vs {mb[k]!r}"


def test_weight_zero_is_the_step_without_the_keyword_autoencoder(pkg, device):
    a, b = _twins(pkg, device, pkg.Networks.Autoencoder, [{}, {"lambda_ssim": 0.0}])
    assert b.image_terms == ()
    x, _ = pkg.synth.batch(2, 32, SEED)
    xb = torch.from_numpy(x).to(device)
    _same_bits(a.training_step({"x": xb, "y": xb}), b.training_step({"x": xb, "y": xb}))
    assert torch.equal(a.optimizer.flat_param, b.optimizer.flat_param)


def _cycle_batch(pkg, device):
    return {"x": pkg.ops.rand_uniform((1, 3, 256, 256), device, seed=SEED, offset=0),
            "y": pkg.ops.rand_uniform((1, 3, 256, 256), device, seed=SEED, offset=1 << 20)}


def test_weight_zero_is_the_step_without_the_keyword_cyclevaegan(pkg, device):
    a, b = _twins(pkg, device, lambda: pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False), [{}, {"lambda_ssim": 0.0}])
    assert b.image_terms == ()
    batch = _cycle_batch(pkg, device)
    pkg.ops.manual_seed(SEED)
    ma = a.training_step(batch)
    pkg.ops.manual_seed(SEED)
    mb = b.training_step(batch)
    assert "loss_ssim" not in mb
    _same_bits(ma, mb)
    assert torch.equal(a.optimizer_G.flat_param, b.optimizer_G.flat_param)
    assert torch.equal(a.optimizer_D.flat_param, b.optimizer_D.flat_param)


# ------------------------------------------------------------------ 8. the cycle models' wiring
@pytest.mark.parametrize("name", ["CycleVAEGAN", "CycleAEGAN"])
def test_cycle_models_add_the_structural_cycle_term(name, pkg, device):
    make = (lambda: pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False)) if name == "CycleVAEGAN" else \
        (lambda: pkg.Networks.CycleAEGAN(paired=False))
    on, off = _twins(pkg, device, make, [{"lambda_ssim": 0.5}, {}])
    batch = _cycle_batch(pkg, device)
    state = {k: v.clone() for k, v in on.state_dict().items()}
    pkg.ops.manual_seed(SEED)
    with torch.no_grad():
        outs = on(batch["x"], batch["y"])
    FGx, GFy = outs[1].detach().cpu().to(torch.float64), outs[3].detach().cpu().to(torch.float64)
    on.load_state_dict(state)                  # the forward advanced the discriminators' power iteration: put u, v back
    pkg.ops.manual_seed(SEED)
    m_on = on.training_step(batch)
    pkg.ops.manual_seed(SEED)
    m_off = off.training_step(batch)
    x64, y64 = batch["x"].cpu().to(torch.float64), batch["y"].cpu().to(torch.float64)
    want = float(ssim_loss_ref(FGx, x64) + ssim_loss_ref(GFy, y64))
    print(f"{name}: loss_ssim {m_on['loss_ssim']:.7f} float64 {want:.7f}; G_loss {m_on['G_loss']:.6f} twin {m_off['G_loss']:.6f}")
    assert list(m_on) == list(m_off) + ["loss_ssim"]
    assert abs(m_on["loss_ssim"] - want) <= 2e-5
    expect = m_off["G_loss"] + 0.5 * m_on["loss_ssim"]
    assert abs(m_on["G_loss"] - expect) <= 1e-3 * max(abs(expect), 1e-6)
    assert m_on["D_loss"] == m_off["D_loss"]
    assert m_on["total_loss"] == m_on["G_loss"] + m_on["D_loss"]
