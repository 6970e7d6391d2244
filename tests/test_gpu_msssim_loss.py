"""GPU: the multi-scale structural loss (csrc/msssim_loss.hip, ops.msssim_loss, lambda_msssim of the models) against a float64
torch restatement of its definition, differentiated by torch autograd on the CPU: conv2d with the outer product of the normalised
Gaussian, avg_pool2d(2) between the levels, clamp(min=1e-4) on the per-image, per-channel factors.  The same function evaluated
in float32 on the CPU is the yardstick of the bounds: the loss to max(1e-5, 4 x float32's error), the gradient to
max(1e-4 of its largest magnitude, 4 x float32's error) — the structural loss's bounds and assert_grad_checksum's margin.

Every case prints its figures as an MSSSIMTABLE line before it asserts (profiles/msssim_loss_accuracy.txt holds them)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import SEED

pytestmark = pytest.mark.gpu

LR = 2e-4
FLOOR = 1e-4
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
# (N, H, W, K): one position at the coarse level; odd sizes with a dropped row and column; ragged tiles on every level and several
# tiles per image; full depth at the minimum size and off it
CASES = [(2, 22, 22, 2), (2, 23, 27, 2), (2, 45, 52, 3), (1, 176, 176, 5), (1, 181, 203, 5)]
SIGMAS = (0.05, 0.3)


def case_id(c):
    return "x".join(map(str, c))


# ------------------------------------------------------------------ the reference
def window(dtype):
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-d * d / (2.0 * 1.5 * 1.5))
    return (g / g.sum()).to(dtype)


def msssim_ref(a, b, scales):
    """(1 - mean MS-SSIM, the (scales, N, 3) factors before the clamp) of (N, 3, H, W) tensors in their own dtype."""
    w = window(a.dtype)
    k = torch.outer(w, w)[None, None].repeat(3, 1, 1, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    total = sum(WEIGHTS[:scales])
    ms, factors = 1.0, []
    for j in range(scales):
        mu_a, mu_b = F.conv2d(a, k, groups=3), F.conv2d(b, k, groups=3)
        s_a = F.conv2d(a * a, k, groups=3) - mu_a * mu_a
        s_b = F.conv2d(b * b, k, groups=3) - mu_b * mu_b
        s_ab = F.conv2d(a * b, k, groups=3) - mu_a * mu_b
        v = (2 * s_ab + c2) / (s_a + s_b + c2)
        if j == scales - 1:
            v = v * (2 * mu_a * mu_b + c1) / (mu_a * mu_a + mu_b * mu_b + c1)
        f = v.mean(dim=(2, 3))
        factors.append(f)
        ms = ms * f.clamp(min=FLOOR) ** (WEIGHTS[j] / total)
        if j < scales - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return 1 - ms.mean(), torch.stack(factors)


def ref_value_and_grad(a, b, scales, dtype):
    x = a.to(dtype).clone().requires_grad_(True)
    loss, factors = msssim_ref(x, b.to(dtype), scales)
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g.to(torch.float64), factors.detach()


def run_op(pkg, a, b, scales, device, gout=None):
    """ops.msssim_loss on fp32 copies of a, b -> (loss, d loss / d a on the CPU in float64, the loss tensor)."""
    x = a.to(torch.float32).to(device).requires_grad_(True)
    loss = pkg.ops.msssim_loss(x, b.to(torch.float32).to(device), scales)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    if gout is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(gout, dtype=torch.float32, device=device))
    return float(loss.detach()), x.grad.detach().cpu().to(torch.float64), loss


def images(n, h, w, sigma, tag=0):
    """b = 0.5 (3 x 3 reflect-padded box blur of u) + 0.5 u, u uniform on [0, 1]; a = b + sigma randn.  Both ARE fp32 numbers:
    every evaluation sees the same values."""
    gen = torch.Generator().manual_seed(SEED + 97 * n + 13 * h + w + 1000 * tag)
    u = torch.rand((n, 3, h, w), generator=gen, dtype=torch.float64)
    b = 0.5 * F.avg_pool2d(F.pad(u, (1, 1, 1, 1), mode="reflect"), 3, stride=1) + 0.5 * u
    a = b + sigma * torch.randn((n, 3, h, w), generator=gen, dtype=torch.float64)
    return a.to(torch.float32).to(torch.float64), b.to(torch.float32).to(torch.float64)


_REFS = {}


def references(key, a, b, scales):
    """float64 and float32 value and gradient of a case, computed once per session."""
    if key not in _REFS:
        _REFS[key] = (ref_value_and_grad(a, b, scales, torch.float64), ref_value_and_grad(a, b, scales, torch.float32))
    return _REFS[key]


def assert_within_bounds(tag, loss, g, r64, r32):
    """The bounds of the module docstring; prints the figures first."""
    (ref, gref, _), (l32, g32, _) = r64, r32
    amax = gref.abs().max().item()
    e_loss, e32_loss = abs(loss - ref), abs(l32 - ref)
    e_grad, e32_grad = (g - gref).abs().max().item(), (g32 - gref).abs().max().item()
    b_loss, b_grad = max(1e-5, 4 * e32_loss), max(1e-4 * amax, 4 * e32_grad)
    print(f"MSSSIMTABLE {tag:26s} loss {loss:.8f} err hip {e_loss:.2e} f32 {e32_loss:.2e} bound {b_loss:.2e} "
          f"({'f32' if 4 * e32_loss > 1e-5 else '1e-5'} binds) | grad amax {amax:.3e} err/amax hip {e_grad / amax:.2e} "
          f"f32 {e32_grad / amax:.2e} bound {b_grad / amax:.2e} ({'f32' if 4 * e32_grad > 1e-4 * amax else '1e-4'} binds)")
    assert torch.isfinite(g).all() and np.isfinite(loss)
    assert e_loss <= b_loss
    assert e_grad <= b_grad


# ------------------------------------------------------------------ 1. value and gradient
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_loss_and_gradient_match_float64(case, sigma, pkg, device):
    n, h, w, scales = case
    a, b = images(n, h, w, sigma)
    r64, r32 = references((case, sigma), a, b, scales)
    fmin = r64[2].min().item()
    print(f"{case} sigma {sigma}: smallest factor {fmin:.3f}")
    assert fmin >= 0.1                                             # the precondition: no case sits near the clamp
    loss, g, _ = run_op(pkg, a, b, scales, device)
    assert_within_bounds(f"{case_id(case)} s={sigma}", loss, g, r64, r32)


# ------------------------------------------------------------------ 2. one scale is the structural loss
@pytest.mark.parametrize("shape", [(2, 23, 27), (2, 45, 52)], ids=case_id)
def test_one_scale_is_the_structural_loss(shape, pkg, device):
    a, b = images(*shape, 0.3, tag=1)
    loss, g, _ = run_op(pkg, a, b, 1, device)
    x = a.to(torch.float32).to(device).requires_grad_(True)
    want = pkg.ops.ssim_loss(x, b.to(torch.float32).to(device))
    want.backward()
    want, gw = float(want.detach()), x.grad.cpu().to(torch.float64)
    print(f"{shape}: msssim(K=1) {loss:.8f} ssim {want:.8f}; gradient max diff / amax {(g - gw).abs().max().item() / gw.abs().max().item():.2e}")
    assert abs(loss - want) <= 1e-6
    assert (g - gw).abs().max().item() <= 1e-5 * gw.abs().max().item()


# ------------------------------------------------------------------ 3. the clamp
@pytest.mark.parametrize("sigma", SIGMAS)
def test_a_clamped_image_passes_no_gradient_and_does_not_leak(sigma, pkg, device):
    n, h, w, scales = 2, 45, 52, 3
    a, b = images(n, h, w, sigma, tag=2)
    ordinary = run_op(pkg, a, b, scales, device)[1]
    a_cl = a.clone()
    a_cl[0] = 1.0 - b[0]                                           # contrast-structure about -0.9: every factor of image 0 far below FLOOR
    a_cl = a_cl.to(torch.float32).to(torch.float64)
    r64, r32 = references(("clamp", sigma), a_cl, b, scales)
    assert r64[2][:, 0].max().item() < -0.5 and r64[2][:, 1].min().item() >= 0.1
    loss, g, _ = run_op(pkg, a_cl, b, scales, device)
    assert_within_bounds(f"clamp 2x45x52x3 s={sigma}", loss, g, r64, r32)
    assert (g[0] == 0).all()                                       # all of image 0's factors are clamped
    assert torch.equal(g[1], ordinary[1])                          # image 1 as in the batch of two ordinary images, bit for bit


# ------------------------------------------------------------------ 4. a = b
@pytest.mark.parametrize("case", [(2, 23, 27, 2), (2, 45, 52, 3), (1, 176, 176, 5)], ids=case_id)
def test_identical_images_give_zero_loss_and_a_finite_gradient(case, pkg, device):
    n, h, w, scales = case
    a, _ = images(n, h, w, 0.05, tag=3)
    loss, g, _ = run_op(pkg, a, a.clone(), scales, device)
    assert abs(loss) <= 1e-6
    assert torch.isfinite(g).all()


# ------------------------------------------------------------------ 5. determinism, scaling, batch independence, the pad channel
def abi_bwd(pkg, a, b, scales, device, gout):
    """vcg_msssim_loss_fwd / _bwd on physical buffers, the gradient buffer poisoned beforehand -> (N, H, W, 4) on the CPU."""
    ap = pkg.ops.as_phys(a.to(torch.float32).to(device))
    bp = pkg.ops.as_phys(b.to(torch.float32).to(device))
    n, h, w, _ = ap.shape
    lib = pkg._native.lib()
    ws = torch.empty(lib.vcg_msssim_loss_workspace(n, h, w, scales) // 4, dtype=torch.float32, device=device)
    out = torch.empty((), dtype=torch.float32, device=device)
    ga = torch.full_like(ap, float("nan"))
    g = torch.tensor([gout], dtype=torch.float32, device=device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pkg._native.check(lib.vcg_msssim_loss_fwd(P(ap), P(bp), P(out), n, h, w, scales, P(ws), ws.numel() * 4, st), "vcg_msssim_loss_fwd")
    pkg._native.check(lib.vcg_msssim_loss_bwd(P(ap), P(bp), P(g), P(ga), n, h, w, scales, P(ws), ws.numel() * 4, st),
                      "vcg_msssim_loss_bwd")
    return ga.cpu()


def test_same_bits_scaling_batch_independence_and_the_pad_channel(pkg, device):
    n, h, w, scales = 3, 45, 52, 3
    a, b = images(n, h, w, 0.3, tag=4)
    l1, g1, t1 = run_op(pkg, a, b, scales, device)
    l2, g2, t2 = run_op(pkg, a, b, scales, device)
    assert torch.equal(t1, t2) and torch.equal(g1, g2)
    amax = g1.abs().max().item()
    _, g37, _ = run_op(pkg, a, b, scales, device, gout=0.37)
    assert (g37 - 0.37 * g1).abs().max().item() <= 1e-6 * 0.37 * amax
    _, g_alone, _ = run_op(pkg, a[:1], b[:1], scales, device)
    assert (n * g1[:1] - g_alone).abs().max().item() <= 1e-6 * g_alone.abs().max().item()
    for gout in (1.0, 0.37):
        phys = abi_bwd(pkg, a, b, scales, device, gout)
        assert torch.isfinite(phys).all() and (phys[..., 3] == 0).all()
    assert torch.equal(abi_bwd(pkg, a, b, scales, device, 1.0)[..., :3].permute(0, 3, 1, 2).to(torch.float64), g1)


# ------------------------------------------------------------------ 6. refusals
def test_bad_sizes_scales_devices_and_channel_counts_are_refused(pkg, device):
    a = torch.rand(1, 3, 175, 180, device=device)
    with pytest.raises(RuntimeError, match="at most 4 scales"):
        pkg.ops.msssim_loss(a, a.clone(), 5)
    a = torch.rand(1, 3, 30, 21, device=device)
    with pytest.raises(RuntimeError, match="at most 1 scales"):
        pkg.ops.msssim_loss(a, a.clone(), 2)
    a = torch.rand(1, 3, 32, 32, device=device)
    for bad in (0, 6, 2.5, True):
        with pytest.raises(RuntimeError, match="scales"):
            pkg.ops.msssim_loss(a, a.clone(), bad)
    with pytest.raises(RuntimeError, match="cuda"):
        pkg.ops.msssim_loss(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 32), 2)
    a = torch.rand(2, 1, 32, 32, device=device)
    with pytest.raises(RuntimeError, match=r"\(N, 3, H, W\)"):
        pkg.ops.msssim_loss(a, a.clone(), 2)
    a = torch.rand(1, 3, 32, 32, device=device)
    with pytest.raises(RuntimeError, match="target"):
        pkg.ops.msssim_loss(a, a.clone().requires_grad_(True), 2)


# ------------------------------------------------------------------ 7. in the step
# G_loss as the weighted sum of the reported terms (configure_loss's defaults; the cycle model unpaired)
STEP_WEIGHTS = {"autoencoder": {"loss_trans": 1.0}, "cyclevaegan": {"loss_cycle": 10.0, "loss_gan_g": 1.0, "loss_kl": 1e-5}}
# batch 2, msssim_scales 2; 32 x 32 for the autoencoder, 256 x 256 for the cycle model: the only square its discriminators accept
STEP_SIZE = {"autoencoder": 32, "cyclevaegan": 256}
LAMBDA = 0.5


def _make(pkg, name):
    return pkg.Networks.Autoencoder() if name == "autoencoder" else pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False)


def _twins(pkg, device, name, configure):
    """Models with equal weights, one per `configure` entry."""
    torch.manual_seed(SEED)
    first = _make(pkg, name)
    sd = {k: v.clone() for k, v in first.state_dict().items()}
    out = []
    for i, kw in enumerate(configure):
        m = first if i == 0 else _make(pkg, name)
        m.load_state_dict(sd)
        m = m.to(device).train()
        m.configure_optimizers(lr=LR)
        m.configure_loss(**kw)
        out.append(m)
    return out, sd


def _batch(pkg, name, device):
    x, y = pkg.synth.batch(2, STEP_SIZE[name], SEED)
    return {"x": torch.from_numpy(x).to(device), "y": torch.from_numpy(y).to(device)}


def _same_bits(ma, mb):
    assert list(ma) == list(mb), f"metric keys {list(ma)} vs {list(mb)}"
    for k in ma:
        assert np.float64(ma[k]).tobytes() == np.float64(mb[k]).tobytes(), f"{k}: {ma[k]!r} vs {mb[k]!r}"


@pytest.mark.parametrize("name", ["autoencoder", "cyclevaegan"])
def test_weight_zero_is_the_step_without_the_keyword(name, pkg, device):
    (zero, plain), _ = _twins(pkg, device, name, [{"lambda_msssim": 0.0, "msssim_scales": 2}, {}])
    assert zero.image_terms == ()
    batch = _batch(pkg, name, device)
    for m in (zero, plain):
        pkg.ops.manual_seed(SEED)
        m.seen = [m.training_step(batch), m.training_step(batch)]
    for ma, mb in zip(zero.seen, plain.seen):
        assert "loss_msssim" not in ma
        _same_bits(ma, mb)
    for opt in zero._opt_names:
        assert torch.equal(getattr(zero, opt).flat_param.view(torch.int32), getattr(plain, opt).flat_param.view(torch.int32))


@pytest.mark.parametrize("name", ["autoencoder", "cyclevaegan"])
def test_the_term_is_reported_last_and_enters_the_generator_loss(name, pkg, device):
    (on, both, plain), sd = _twins(pkg, device, name, [{"lambda_msssim": LAMBDA, "msssim_scales": 2},
                                                       {"lambda_msssim": LAMBDA, "msssim_scales": 2, "lambda_ssim": 0.25, "lambda_freq": 0.25},
                                                       {}])
    batch = _batch(pkg, name, device)
    # the term on the model's own operands: the autoencoder's returned output; the cycle model's F(G(x)), G(F(y)) of its forward
    pkg.ops.manual_seed(SEED)
    v_on = on.validation_step(batch)
    if name == "autoencoder":
        want = float(pkg.ops.msssim_loss(v_on["Gx"], batch["y"], 2))
    else:
        pkg.ops.manual_seed(SEED)
        with torch.no_grad():
            outs = on(batch["x"], batch["y"])                        # Gx, FGx, Fy, GFy, ...
        want = float(pkg.ops.msssim_loss(outs[1], batch["x"], 2)) + float(pkg.ops.msssim_loss(outs[3], batch["y"], 2))
        on.load_state_dict(sd)                                       # the forward advanced the discriminators' power iteration
    print(f"{name}: validation loss_msssim {v_on['loss_msssim']:.8f}, the op on the model's operands {want:.8f}")
    assert abs(v_on["loss_msssim"] - want) <= 2e-5
    pkg.ops.manual_seed(SEED)
    v_both = both.validation_step(batch)
    assert [k for k in v_both if k not in ("Gx", "Fy")][-3:] == ["loss_ssim", "loss_freq", "loss_msssim"]
    pkg.ops.manual_seed(SEED)
    m_on = on.training_step(batch)
    pkg.ops.manual_seed(SEED)
    m_plain = plain.training_step(batch)
    assert [k for k in m_on if k not in m_plain] == ["loss_msssim"] and list(m_on)[:len(m_plain)] == list(m_plain)
    for what, m in (("training_step", m_on), ("validation_step", v_on)):
        expect = sum(wt * m[k] for k, wt in STEP_WEIGHTS[name].items()) + LAMBDA * m["loss_msssim"]
        print(f"{name} {what}: G_loss {m['G_loss']:.7f}, weighted sum {expect:.7f}")
        assert abs(m["G_loss"] - expect) <= 1e-3 * abs(expect)
    if name == "cyclevaegan":
        assert np.float64(m_on["D_loss"]).tobytes() == np.float64(m_plain["D_loss"]).tobytes()
        assert m_on["total_loss"] == m_on["G_loss"] + m_on["D_loss"]
    assert not torch.equal(getattr(on, on._opt_names[0]).flat_param, getattr(plain, plain._opt_names[0]).flat_param)
