"""GPU: the discriminator head above 256 x 256 — vcg_patch_head_fwd / _dgrad / _wgrad (csrc/patch_head.hip), their dispatch in
ops.fullmap_sn_conv, and one step of the GAN models at 272 x 256.

1. The three entry points against float64, through the C ABI, at the smallest shapes at which each thing can go wrong (CASES).
   The operands handed to the kernels (x, g, the wsn_k vcg_sn_prepare wrote) are exact inputs, so the bounds are the
   arithmetic's alone: a sum of L fp32 products accumulated in fp32 in any order is within (L + 2) 2^-24 sum|products| of the
   exact sum — L = KH KW C for a logit (plus one rounding of the result when the bias is added), the number of contributing
   logits for an element of dx, N OH OW for gk.  The weight gradient's spectral-norm stage keeps the bound test_fullmap_conv of
   tests/test_gpu_norm_misc.py gives it, with N OH OW addends in place of N.  Outputs are prefilled with NaN and followed by
   sentinel words; the forward runs twice (same bits); image 1 of the batch-2 case alone gives image 1's bits.
2. ops.fullmap_sn_conv on a 512 x 17 x 16 map, batch 2, against the float64 restatement `_sn_ref` (as in
   tests/test_gpu_autograd_routes.py, which is size-generic), every gradient route, train and eval, and two traversals.
3. Dispatch: a 16 x 16 map gives the bits of vcg_sn_prepare + vcg_fullmap_fwd; a smaller map raises.
4. One training and one validation step at 272 x 256, batch 1: CycleVAEGAN (unpaired) and AEGAN against the float64 oracle;
   CycleVAEGAN with pool_size=4; then a 256 x 256 step bitwise equal to a twin's that never saw 272 x 256.
"""
import importlib
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import SEED, assert_close, assert_grad_checksum, assert_param_after_step, checksum, in_cancelled_bias
from test_gpu_norm_misc import Out, P, U, _call, _randn, _sn_depth, _sn_run, _st, _worst, _ws, nchw, nhwc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from cases import LR, STEP_BIAS_STD  # noqa: E402

pytestmark = pytest.mark.gpu

# (N, C, KH, KW, H, W)
CASES = [(2, 8, 3, 3, 5, 4),          # a few taps, small enough to check by eye
         (3, 12, 4, 4, 4, 7),         # a single output row, C not a power of two
         (1, 8, 2, 2, 3, 40),         # OW = 39: past any 32-wide tile edge
         (1, 512, 16, 16, 17, 16),    # the real head at 272 x 256
         (2, 512, 16, 16, 18, 19)]    # the real head, non-square, batch 2
CASES.append((1, 4, 17, 18, 19, 20))   # beyond the issue's table: a kernel above one 16 x 16 matrix tile (two ky and two kx tiles)


def _ws_bytes(pkg, N, H, W, C, KH, KW):
    n = pkg._native.lib().vcg_patch_head_workspace(N, H, W, C, KH, KW)
    assert n > 0 and n % 16 == 0
    return n


def _fwd(pkg, x, wsn, bias, N, H, W, C, KH, KW, device):
    OH, OW = H - KH + 1, W - KW + 1
    out = Out((N * OH * OW,), device)
    ws = _ws(_ws_bytes(pkg, N, H, W, C, KH, KW), device)
    _call(pkg, "vcg_patch_head_fwd", P(x), P(wsn), P(bias), P(out.t), N, H, W, C, KH, KW, P(ws), ws.numel() * 4, _st())
    torch.cuda.synchronize()
    return out.check("vcg_patch_head_fwd")


def _dgrad(pkg, g, wsn, N, H, W, C, KH, KW, device):
    dx = Out((N, H, W, C), device)
    _call(pkg, "vcg_patch_head_dgrad", P(g), P(wsn), P(dx.t), N, H, W, C, KH, KW, _st())
    torch.cuda.synchronize()
    return dx.check("vcg_patch_head_dgrad")


@pytest.mark.parametrize("case", CASES, ids=["N{}_{}x{}x{}_map{}x{}".format(*c) for c in CASES])
def test_patch_head_entry_points_match_float64(case, pkg, device):
    N, C, KH, KW, H, W = case
    OH, OW = H - KH + 1, W - KW + 1
    K, G = C * KH * KW, N * OH * OW
    w = _randn((1, C, KH, KW), device, 240 + C) * 0.05
    u, v, sigma, wsn = _sn_run(pkg, w, 0.6, torch.zeros(K, device=device), C, KH, KW, 1, device)
    x = _randn((N, H, W, C), device, 241 + N)
    g = _randn((G,), device, 242 + N)
    bias = torch.tensor([0.3], device=device)
    # ---- forward: float64 from the fp32 operands the kernel reads
    wk64 = wsn.double().reshape(KH, KW, C).permute(2, 0, 1)[None]                         # (1, C, KH, KW)
    x64 = nchw(x).double()
    out = _fwd(pkg, x, wsn, bias, N, H, W, C, KH, KW, device)
    again = _fwd(pkg, x, wsn, bias, N, H, W, C, KH, KW, device)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two forward calls differ"
    o = F.conv2d(x64, wk64).reshape(-1) + 0.3
    prod = F.conv2d(x64.abs(), wk64.abs()).reshape(-1)
    assert out.shape == (G,)
    assert _worst((out.double() - o).abs(), (K + 2) * U * prod + U * (o.abs() + 0.3), "patch_head_fwd") <= 1
    # ---- data gradient: every element written (NaN prefill), L = the logits that reach it
    dx = _dgrad(pkg, g, wsn, N, H, W, C, KH, KW, device)
    assert not torch.isnan(dx).any(), "vcg_patch_head_dgrad left elements of dx unwritten"
    g64 = g.double().reshape(N, 1, OH, OW)
    dref = nhwc(F.conv_transpose2d(g64, wk64))
    dprod = nhwc(F.conv_transpose2d(g64.abs(), wk64.abs()))
    reach = nhwc(F.conv_transpose2d(torch.ones_like(g64), torch.ones_like(wk64)))         # contributing logits per element
    assert _worst((dx.double() - dref).abs(), (reach + 2) * U * dprod + 1e-300, "patch_head_dgrad") <= 1
    # ---- weight gradient: float64 autograd of conv2d(x, W / sigma) + b, sigma = u . W v with u, v constants
    pre_w, pre_b = _randn((1, C, KH, KW), device, 243) * 1e-3, torch.tensor([0.25], device=device)
    gw, gb = Out((1, C, KH, KW), device, fill=pre_w), Out((1,), device, fill=pre_b)
    ws = _ws(_ws_bytes(pkg, N, H, W, C, KH, KW), device)
    _call(pkg, "vcg_patch_head_wgrad", P(g), P(x), P(wsn), P(sigma), P(u), P(v), P(gw.t), P(gb.t), N, H, W, C, KH, KW, P(ws),
          ws.numel() * 4, _st())
    torch.cuda.synchronize()
    Wp = w.double().requires_grad_(True)
    sig = u.double() * (Wp.reshape(1, -1) @ v.double())
    F.conv2d(x64, Wp / sig, bias.double()).reshape(-1).backward(g.double())
    L = _sn_depth(K)
    sg_tol = (2 * L + 16) * U
    # A[c, ky, kx] = sum_{n,oy,ox} |g x|: the correlation of |x| with |g|, images as channels
    A = F.conv2d(x64.abs().transpose(0, 1), g64.abs().transpose(0, 1)).transpose(0, 1)     # (1, C, KH, KW)
    B = (A * Wp.detach().abs()).sum() / sig.detach().abs()
    scale = (A + B * (u.double() * v.double().reshape(1, C, KH, KW)).abs()) / sig.detach().abs()
    ref = pre_w.double() + Wp.grad
    tol = (G + L + sg_tol / U + 16) * U * scale + 2 * U * ref.abs()
    assert _worst((gw.check("vcg_patch_head_wgrad gw").double() - ref).abs(), tol + 1e-300, "patch_head_wgrad gw") <= 1
    bref = 0.25 + g.double().sum().item()
    assert abs(gb.check("vcg_patch_head_wgrad gbias").double().item() - bref) <= (G + 1) * U * (g.double().abs().sum().item() + 0.25 + abs(bref))
    # ---- an image's results do not depend on the rest of the batch
    if N == 2:
        o1 = _fwd(pkg, x[1:].contiguous(), wsn, bias, 1, H, W, C, KH, KW, device)
        assert torch.equal(o1.view(torch.int32), out[OH * OW:].view(torch.int32)), "image 1's logits depend on image 0"
        d1 = _dgrad(pkg, g[OH * OW:].contiguous(), wsn, 1, H, W, C, KH, KW, device)
        assert torch.equal(d1.view(torch.int32), dx[1:].view(torch.int32)), "image 1's dx depends on image 0"


def test_a_wide_map_gives_a_shard_the_bits_of_the_batch(pkg, device):
    """A 130-pixel-wide map with 64 channels: a row slab of ONE image fits the widest channel chunk, that of two images does
    not, so a chunk width taken from the batch would add another number of partials at N = 1 than at N = 2."""
    N, C, KH, KW, H, W = 2, 64, 2, 2, 3, 130
    OH, OW = H - KH + 1, W - KW + 1
    wsn = _randn((KH * KW * C,), device, 250) * 0.05
    x = _randn((N, H, W, C), device, 251)
    g = _randn((N * OH * OW,), device, 252)
    bias = torch.tensor([0.3], device=device)
    out = _fwd(pkg, x, wsn, bias, N, H, W, C, KH, KW, device)
    dx = _dgrad(pkg, g, wsn, N, H, W, C, KH, KW, device)
    for i in range(N):
        oi = _fwd(pkg, x[i:i + 1].contiguous(), wsn, bias, 1, H, W, C, KH, KW, device)
        assert torch.equal(oi.view(torch.int32), out[i * OH * OW:(i + 1) * OH * OW].view(torch.int32)), f"image {i}: logits"
        di = _dgrad(pkg, g[i * OH * OW:(i + 1) * OH * OW].contiguous(), wsn, 1, H, W, C, KH, KW, device)
        assert torch.equal(di.view(torch.int32), dx[i:i + 1].view(torch.int32)), f"image {i}: dx"
    o = F.conv2d(nchw(x).double(), wsn.double().reshape(KH, KW, C).permute(2, 0, 1)[None]).reshape(-1) + 0.3
    prod = F.conv2d(nchw(x).double().abs(), wsn.double().abs().reshape(KH, KW, C).permute(2, 0, 1)[None]).reshape(-1)
    assert _worst((out.double() - o).abs(), (KH * KW * C + 2) * U * prod + U * (o.abs() + 0.3), "patch_head_fwd wide") <= 1


# ====================================================================================================================== 2
def _data(pkg, device, shape, key, scale=1.0):
    return (torch.from_numpy(pkg.synth.normal(tuple(shape), SEED, "patch_head/" + key)) * scale).to(device)


def _sn_setup(pkg, device):
    C, KH, KW, N, H, W = 512, 16, 16, 2, 17, 16
    w0 = _data(pkg, device, (1, C, KH, KW), "w", 0.05)
    v0 = F.normalize(_data(pkg, device, (C * KH * KW,), "v"), dim=0)
    x0 = _data(pkg, device, (N, C, H, W), "x")
    g0 = _data(pkg, device, (N * (H - KH + 1) * (W - KW + 1),), "g")
    return w0, torch.tensor([1.0], device=device), v0, torch.tensor([0.3], device=device), x0, g0


def _sn_ref(x64, w64, b64, u, v, training):
    """float64, with u, v as they are AFTER the forward's power iteration (training) or as given (eval), both constants."""
    wm = w64.reshape(1, -1)
    if training:
        with torch.no_grad():
            v = F.normalize(torch.mv(wm.detach().t(), u.double()), dim=0, eps=1e-12)
            u = F.normalize(torch.mv(wm.detach(), v), dim=0, eps=1e-12)
    sigma = torch.dot(u.double(), torch.mv(wm, v.double()))
    return F.conv2d(x64, w64 / sigma, b64).reshape(-1)


def _nchw(ops, t):
    return ops.to_nchw_contiguous(t.detach())


@pytest.mark.parametrize("mode", ["all", "x detached", "weight frozen", "no_wgrad"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_fullmap_sn_conv_on_a_larger_map_gradient_subsets(training, mode, pkg, device):
    ops = pkg.ops
    w0, u0, v0, b0, x0, g0 = _sn_setup(pkg, device)
    w, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    u, v = u0.clone(), v0.clone()
    w64, b64 = w0.double().requires_grad_(mode != "weight frozen"), b0.double().requires_grad_(True)
    if mode == "weight frozen":
        w.requires_grad_(False)
    x = ops.to_nhwc(x0).requires_grad_(mode != "x detached")
    x64 = x0.double().requires_grad_(mode != "x detached")
    out = ops.fullmap_sn_conv(x, w, b, u, v, training)
    assert out.shape == (2 * 2 * 1,)
    ref = _sn_ref(x64, w64, b64, u0, v0, training)
    if mode == "no_wgrad":
        with ops.no_wgrad([w, b]):
            out.backward(g0)
    else:
        out.backward(g0)
    ref.backward(g0.double())
    assert_close(out.detach(), ref.detach(), "patch head y")
    if training:
        assert not torch.equal(v, v0), "training mode advances v in place"
    else:
        assert torch.equal(v, v0) and torch.equal(u, u0)
    if mode == "x detached":
        assert x.grad is None
    else:
        assert_close(_nchw(ops, x.grad), x64.grad, "patch head dx")
    if mode == "no_wgrad":
        assert w.grad is None and b.grad is None
    elif mode == "weight frozen":
        assert w.grad is None
        assert_close(b.grad, b64.grad, "patch head dbias under a frozen weight")
    else:
        assert_close(w.grad, w64.grad, "patch head dweight")
        assert_close(b.grad, b64.grad, "patch head dbias")


def test_fullmap_sn_conv_on_a_larger_map_differentiated_twice(pkg, device):
    ops = pkg.ops
    w0, u0, v0, b0, x0, g0 = _sn_setup(pkg, device)
    w, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    u, v = u0.clone(), v0.clone()
    x, x64 = ops.to_nhwc(x0).requires_grad_(True), x0.double().requires_grad_(True)
    w64, b64 = w0.double().requires_grad_(True), b0.double().requires_grad_(True)
    out = ops.fullmap_sn_conv(x, w, b, u, v, True)
    ref = _sn_ref(x64, w64, b64, u0, v0, True)
    out.backward(g0, retain_graph=True)
    ref.backward(g0.double(), retain_graph=True)
    first = (_nchw(ops, x.grad).clone(), w.grad.clone(), b.grad.clone())
    v_then = v.clone()
    with torch.no_grad():
        w.add_(_data(pkg, device, tuple(w.shape), "w step", 0.05))
        ops.fullmap_sn_conv(ops.to_nhwc(x0), w, b, u, v, True)
    assert not torch.equal(v, v_then)
    out.backward(g0)
    ref.backward(g0.double())
    assert_close(_nchw(ops, x.grad), x64.grad, "dx after two traversals")
    assert_close(w.grad, w64.grad, "dweight after two traversals")
    assert_close(b.grad, b64.grad, "dbias after two traversals")
    assert_close(_nchw(ops, x.grad) - first[0], first[0], "the second traversal's dx")
    assert_close(w.grad - first[1], first[1], "the second traversal's dweight")
    assert_close(b.grad - first[2], first[2], "the second traversal's dbias")


# ====================================================================================================================== 3
def test_a_map_of_the_kernels_size_takes_the_full_map_kernels(pkg, device):
    ops = pkg.ops
    C, KH, KW, N = 512, 16, 16, 2
    w0 = _data(pkg, device, (1, C, KH, KW), "w", 0.05)
    v0 = F.normalize(_data(pkg, device, (C * KH * KW,), "v"), dim=0)
    x0 = _data(pkg, device, (N, C, KH, KW), "x16")
    bias = torch.tensor([0.3], device=device)
    u, v = torch.tensor([1.0], device=device), v0.clone()
    got = ops.fullmap_sn_conv(ops.to_nhwc(x0), w0, bias, u, v, True)
    _, _, _, wsn = _sn_run(pkg, w0, 1.0, v0, C, KH, KW, 1, device)
    want = Out((N,), device)
    _call(pkg, "vcg_fullmap_fwd", P(ops.as_phys(ops.to_nhwc(x0))), P(wsn), P(bias), P(want.t), N, C * KH * KW, _st())
    torch.cuda.synchronize()
    assert got.shape == (N,) and torch.equal(got.view(torch.int32), want.check("vcg_fullmap_fwd").view(torch.int32))


def test_a_map_smaller_than_the_kernel_is_refused(pkg, device):
    ops = pkg.ops
    w0 = _data(pkg, device, (1, 512, 16, 16), "w", 0.05)
    x0 = torch.zeros(1, 512, 15, 16, device=device)
    with pytest.raises(RuntimeError, match=r"smallest accepted image is 256x256.*reference.*fails"):
        ops.fullmap_sn_conv(ops.to_nhwc(x0), w0, torch.zeros(1, device=device), torch.ones(1, device=device),
                            torch.zeros(512 * 256, device=device), True)


# ====================================================================================================================== 4
LATENT = 64
SIZE = (272, 256)


def _rect_batch(pkg, device, n, hw, step=0):
    """synth.batch draws squares: the 272-row square cropped to 256 columns"""
    x, y = pkg.synth.batch(n, max(hw), SEED, step=step)
    xb, yb = (torch.from_numpy(a)[:, :, :hw[0], :hw[1]].contiguous() for a in (x, y))
    return xb, yb


def _load(pkg, model, seed_shift=0):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = pkg.synth.state_dict_like(shapes, SEED + seed_shift, bias_std=STEP_BIAS_STD)
    sd = {k: torch.from_numpy(v) for k, v in sd.items()}
    model.load_state_dict(sd)
    return sd


def _check_metrics(got, want, what):
    for k, v in want.items():
        assert k in got, (what, k)
        assert abs(got[k] - v) <= 1e-3 * max(abs(v), 1e-6), f"{what}: {k} = {got[k]!r}, float64 oracle {v!r}"


@pytest.mark.parametrize("arch", ["cyclevaegan", "aegan"])
def test_one_step_and_validation_at_272x256_match_float64(arch, pkg, oracle, device):
    """As test_step_at_the_default_batch_sizes_matches_float64 (tests/test_gpu_changing_shapes.py) through
    test_gpu_ssim_loss._check_step: losses and d_*_mean to 1e-3 of the float64 oracle; EVERY parameter gradient of both
    optimizers by conftest.assert_grad_checksum (error against the float64 gradient within max(4 tol, 4 x the float32 oracle's
    own error, FLIP_BUDGET = 1e-2)); every parameter after the step by conftest.assert_param_after_step, which knows that the
    first Adam update is lr sign(g); the spectral-norm vectors by assert_close.  IN-cancelled biases are skipped as everywhere."""
    gan = arch == "cyclevaegan"
    model = pkg.Networks.CycleVAEGAN(latent_dim=LATENT, paired=False) if gan else pkg.Networks.AEGAN()
    sd = _load(pkg, model)
    model = model.to(device).train()
    model.configure_optimizers(lr=LR)
    model.configure_loss()
    xb, yb = _rect_batch(pkg, device, 1, SIZE)
    eps = [torch.from_numpy(e) for e in pkg.synth.eps_list(6, (1, LATENT, SIZE[0] // 16, SIZE[1] // 16), SEED)] if gan else None
    if gan:
        pkg.ops.inject_eps(list(eps))
    got = model.training_step({"x": xb.to(device), "y": yb.to(device)})
    res = {}
    for dtype in (torch.float64, torch.float32):
        Q = {k: v.to(dtype).clone() for k, v in sd.items()}
        if gan:
            want, _, gg, dg = oracle.cyclevaegan_step(Q, {}, xb.to(dtype), yb.to(dtype), [e.to(dtype) for e in eps], LR, paired=False)
        else:
            want, gg, dg = oracle.single_gan_step(Q, {}, xb.to(dtype), yb.to(dtype), None, LR)
        g = dict(gg)
        g.update(dg)
        res[dtype] = (want, g, Q)
    want, g64, P64 = res[torch.float64]
    _, g32, _ = res[torch.float32]
    x64, y64 = xb.double(), yb.double()
    heads = ("DX.", "DY.") if gan else ("D.",)
    _check_metrics(got, want, f"{arch} step at 272x256")
    state = model.state_dict()
    for h in heads:
        for s in ("weight_u", "weight_v"):
            assert_close(state[f"{h}model.4.{s}"], P64[f"{h}model.4.{s}"].float(), f"{h}model.4.{s}")
    bad, checked = [], 0
    key = f"{arch}272x256"
    for n, p in model.named_parameters():
        if in_cancelled_bias(n) or g64.get(n) is None:
            continue
        assert p.grad is not None, f"{n} has no gradient after the step"
        ck32, ck64 = checksum(g32[n].to(device)), checksum(g64[n].to(device))
        try:
            assert_grad_checksum(p.grad, ck32, ck64, "grad " + n, key=key)
            assert_param_after_step(state[n], checksum(P64[n].to(device)), "param " + n, LR, gck32=ck32, gck64=ck64)
        except AssertionError as e:
            bad.append(str(e))
        checked += 1
    print(f"{key}: {checked} parameter tensors checked, {len(bad)} off")
    assert checked >= 20, checked
    assert not bad, f"{len(bad)} of {checked} tensors off:\n" + "\n".join(b[:300] for b in bad[:12])
    # validation (eval mode: the stored u, v; no update)
    model.eval()
    if gan:
        pkg.ops.inject_eps(list(eps))
    v = model.validation_step({"x": xb.to(device), "y": yb.to(device)})
    model.train()
    Pv = {k: t.detach().cpu().double() for k, t in model.state_dict().items()}
    if gan:
        wantv, _ = oracle.cyclevaegan_validation(Pv, x64, y64, [e.double() for e in eps], paired=False)
    else:
        wantv, _ = oracle.single_gan_validation(Pv, x64, y64, None)
    _check_metrics({k: t for k, t in v.items() if not torch.is_tensor(t)}, wantv, f"{arch} validation at 272x256")


def test_a_pooled_step_at_272x256_then_256_matches_a_twin(pkg, device):
    Net = pkg.Networks.CycleVAEGAN

    def make(pool):
        m = Net(latent_dim=LATENT, paired=False)
        _load(pkg, m)
        m = m.to(device).train()
        m.configure_optimizers(lr=LR, pool_size=pool) if pool else m.configure_optimizers(lr=LR)
        m.configure_loss()
        return m

    def step(m, hw, k):
        xb, yb = _rect_batch(pkg, device, 1, hw, step=k)
        eps = [torch.from_numpy(e) for e in pkg.synth.eps_list(6, (1, LATENT, hw[0] // 16, hw[1] // 16), SEED, step=k)]
        pkg.ops.inject_eps(eps)
        return m.training_step({"x": xb.to(device), "y": yb.to(device)})

    pooled = make(4)
    m = step(pooled, SIZE, 0)
    assert isinstance(m["D_loss"], float) and m["D_loss"] == m["D_loss"] and abs(m["D_loss"]) != float("inf"), m
    del pooled
    a, b = make(0), make(0)
    step(a, SIZE, 0)
    snap = ({k: v.detach().clone() for k, v in a.state_dict().items()}, {n: o.state_dict() for n, o in _opts(a).items()})
    b.load_state_dict(snap[0])
    for n, o in _opts(b).items():
        o.load_state_dict(snap[1][n])
    ma, mb = step(a, (256, 256), 1), step(b, (256, 256), 1)
    assert ma == mb, (ma, mb)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{k} differs from the twin that never saw 272x256"


def _opts(model):
    return importlib.import_module("test_gpu_grad_clip")._opts(model)
