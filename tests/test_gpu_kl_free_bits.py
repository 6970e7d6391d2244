"""GPU: the KL term with a free-bits floor (csrc/kl_free_bits.hip, ops.kl_free_bits) against a float64 reference written out
here.

Reference.  k = -0.5 (1 + l - mu^2 - exp(l)), l = clamp(logvar, -10, 10); KL_c = mean of k over batch and positions of channel c;
loss = mean_c max(KL_c, floor), plain = mean_c KL_c, active = #{c: KL_c > floor}; the gradient is torch's float64 autograd of
`loss` with the gate held fixed (max passes the gradient where KL_c > floor).

Inputs.  mu of channel c is scaled by one of two amplitudes so that the channel KLs fall into two groups; a share of the logvar
values sits at and beyond the clamp (+-10, +-12).  The floor is the float32 nearest the middle of the widest gap between
neighbouring channel KLs around their median, so about half of the channels lie on each side; every |KL_c - floor| >= 1e-3 floor is asserted on the host, in float64, before anything is
compared, and so is that every channel's forward error bound is below its distance to the floor (the gates of a correct kernel
then agree with the reference's).  No channel is excluded from any comparison.

Forward bound, per channel, the derivation of test_kl_loss_at_the_clamp_edges (tests/test_gpu_norm_misc.py): unit roundoff x
(depth + const) x sum|terms| / (2 R) + U |KL_c|.  depth: a lane adds its rows serially (rows per lane, below) and the row lanes
of a workgroup meet in a binary tree of at most 8 levels; the slabs and the channels are then summed in double.  const = 8 covers
the four operations and the expf of one term.  out[0] and out[1] are means of the channel values taken in double and rounded
once: the mean of the channel bounds + U |value|.

The launch plan is mirrored in `plan` (the workspace size the library reports checks the mirror): tc channel quads x tp row lanes
per workgroup, rows per lane = ceil(R / (64 tp)), a workgroup covers tp x that many rows."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def plan(rows, c):
    cp4 = (c + 3) // 4
    tc = 1
    while tc < cp4 and tc < 64:
        tc *= 2
    tp = 256 // tc
    rpl = max(1, -(-rows // (tp * 64)))
    slab = tp * rpl
    return {"tp": tp, "rpl": rpl, "slab": slab, "nslab": -(-rows // slab), "cp": cp4 * 4}


def _covered(c):
    return plan(1, c)["slab"]                     # rows one workgroup covers while the rows fit 64 slabs


# (N, C, h, w).  C = 64: 16 row lanes per workgroup -> 15, 16, 17 rows are one fewer than, equal to and one more than a workgroup
# covers; 1031 rows (prime) at C = 64 take two rows per lane in 33 slabs, the last one ragged
SHAPES = [(1, 4, 1, 1), (3, 6, 2, 3), (2, 64, 4, 4), (2, 1024, 2, 2), (1, 64, 3, 5), (1, 64, 4, 4), (1, 64, 1, 17), (1, 64, 1, 1031)]


def test_the_shapes_hit_the_plan_edges(pkg):
    lib = pkg._native.lib()
    assert _covered(64) == 16
    assert [n * h * w for n, c, h, w in SHAPES if c == 64][1:4] == [15, 16, 17]
    for n, c, h, w in SHAPES:
        pl = plan(n * h * w, c)
        assert lib.vcg_kl_fb_workspace(n * h * w, pl["cp"]) == pl["nslab"] * pl["cp"] * 4, (n, c, h, w)
    assert [plan(r, 64)["nslab"] for r in (15, 16, 17)] == [1, 1, 2]
    big = plan(1031, 64)
    assert big["rpl"] == 2 and big["nslab"] == 33 and 1031 % big["slab"] != 0
    assert plan(8, 1024)["tp"] == 4 and plan(8, 1024)["cp"] // 4 // 64 == 4        # four channel groups, two slabs of rows
    assert plan(18, 6)["cp"] == 8


def _inputs(shape, seed, device):
    """(mu, logvar) float32 on the host as NCHW, channel amplitudes in two groups, logvar with values at and beyond the clamp."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    amp = torch.where(torch.arange(c) % 2 == 0, torch.tensor(0.3), torch.tensor(2.0)) * (1 + 0.2 * torch.rand(c, generator=g))
    mu = torch.randn(shape, generator=g) * amp.view(1, c, 1, 1)
    lv = torch.randn(shape, generator=g) * 0.5
    edge = torch.rand(shape, generator=g)
    vals = torch.tensor([-12.0, -10.0, 10.0, 12.0])
    pick = vals[torch.randint(0, 4, shape, generator=g)]
    rows = n * h * w
    lv = torch.where(edge < (0.02 if rows < 100 else 0.001), pick, lv)
    flat = lv.permute(1, 0, 2, 3).reshape(c, -1).clone()
    flat[0, 0] = 12.0                             # every case has a value beyond the clamp; small latents get both sides
    if rows >= 4:
        flat[min(1, c - 1), 1], flat[min(2, c - 1), 2], flat[min(3, c - 1), 3] = -12.0, 10.0, -10.0
    lv = flat.reshape(c, n, h, w).permute(1, 0, 2, 3).contiguous()
    return mu, lv


def reference(mu, lv, floor, gout=1.0):
    """float64: (loss, plain, active, KL_c, gmu, glv, abs-sum per channel) for NCHW or (N, C) float32 host tensors."""
    mu64, lv64 = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    lc = torch.clamp(lv64, -10, 10)
    k = -0.5 * (1 + lc - mu64 ** 2 - torch.exp(lc))
    dims = [d for d in range(mu.dim()) if d != 1]
    klc = k.mean(dim=dims)
    open_ = ~(klc.detach() <= floor)
    loss = torch.where(open_, klc, torch.full_like(klc, floor)).mean()
    (loss * gout).backward()
    rows = mu.numel() // mu.shape[1]
    absum = (0.5 * (1 + lc.abs() + mu64 ** 2 + torch.exp(lc))).detach().sum(dim=dims) / rows
    return (loss.item(), klc.detach().mean().item(), int(open_.sum()), klc.detach(), mu64.grad, lv64.grad, absum)


def median_floor(klc):
    """The float32 nearest the middle of the widest gap between neighbours among the central fifth of the sorted channel KLs."""
    s = torch.sort(klc).values
    c = len(s)
    lo, hi = c // 2 - 1 - c // 10, c // 2 - 1 + c // 10
    i = lo + int(torch.argmax(s[lo + 1:hi + 2] - s[lo:hi + 1]))
    return float(np.float32(0.5 * (s[i] + s[i + 1]).item()))


def channel_bound(shape, klc, absum):
    rows = shape[0] * shape[2] * shape[3]
    depth = plan(rows, shape[1])["rpl"] + 8
    return U * ((depth + 8) * absum + klc.abs())


def assert_margin(klc, floor, bound):
    gap = (klc - floor).abs()
    assert (gap >= 1e-3 * floor).all(), f"test inputs: a channel KL within 1e-3 of the floor {floor}: {gap.min().item():.3e}"
    assert (bound < gap).all(), "test inputs: a channel's forward bound exceeds its distance to the floor"
    below = int((klc <= floor).sum())
    assert 0 < below < len(klc) and abs(below - len(klc) / 2) <= max(1, len(klc) // 8), (below, len(klc))


def to_dev(pkg, t, device):
    return pkg.ops.to_nhwc(t.to(device))


def nchw(t):
    return (t * 1.0).contiguous().cpu()


_CACHE = {}


def case(pkg, device, shape):
    """inputs, float64 reference and the op's results for `shape`, computed once per session."""
    if shape not in _CACHE:
        mu, lv = _inputs(shape, 1000 + sum(shape), device)
        klc0 = reference(mu, lv, 0.0)[3]
        floor = median_floor(klc0)
        ref = reference(mu, lv, floor, gout=1.5)
        mud, lvd = to_dev(pkg, mu, device).requires_grad_(True), to_dev(pkg, lv, device).requires_grad_(True)
        loss, plain, active, klc = pkg.ops.kl_free_bits(mud, lvd, floor, channel_kl=True)
        (loss * 1.5).backward()
        torch.cuda.synchronize()
        _CACHE[shape] = dict(mu=mu, lv=lv, floor=floor, ref=ref, mud=mud, lvd=lvd, loss=loss.item(), plain=plain.item(),
                             active=active.item(), klc=klc.cpu().double(), gmu=nchw(mud.grad), glv=nchw(lvd.grad),
                             gmu_raw=mud.grad, glv_raw=lvd.grad)
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_against_float64(shape, pkg, device):
    cs = case(pkg, device, shape)
    ref_loss, ref_plain, ref_active, ref_klc, _, _, absum = cs["ref"]
    bound = channel_bound(shape, ref_klc, absum)
    assert_margin(ref_klc, cs["floor"], bound)
    err = (cs["klc"] - ref_klc).abs()
    print(f"{shape}: worst klc error / bound {(err / bound).max().item():.3f}; floor {cs['floor']:.4f}; open {ref_active} of {shape[1]}")
    assert (err <= bound).all(), f"klc: worst error / bound {(err / bound).max().item():.3f}"
    assert cs["active"] == ref_active
    open_ = ~(ref_klc <= cs["floor"])
    b0 = (bound * open_).mean().item() + U * abs(ref_loss)
    b1 = bound.mean().item() + U * abs(ref_plain)
    print(f"{shape}: loss error / bound {abs(cs['loss'] - ref_loss) / b0:.3f}, plain error / bound {abs(cs['plain'] - ref_plain) / b1:.3f}")
    assert abs(cs["loss"] - ref_loss) <= b0
    assert abs(cs["plain"] - ref_plain) <= b1
    assert cs["loss"] >= cs["plain"]
    # the plain mean against ops.kl_loss on the same tensors: within the sum of both bounds (kl_loss: one flat reduction of
    # R C terms, test_kl_loss_at_the_clamp_edges's bound with its depth of a 256-lane workgroup's tree over at most 1024 blocks)
    n_all = cs["mu"].numel()
    depth_flat = math.ceil(n_all / (1024 * 256 * 4)) * 4 + 8 + 2
    b_flat = U * ((depth_flat + 6) * absum.mean().item() + abs(ref_plain))
    flat = pkg.ops.kl_loss(cs["mud"].detach(), cs["lvd"].detach()).item()
    assert abs(flat - cs["plain"]) <= b1 + b_flat, (flat, cs["plain"], b1 + b_flat)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_against_float64(shape, pkg, device):
    cs = case(pkg, device, shape)
    _, _, _, ref_klc, gmu64, glv64, _ = cs["ref"]
    n, c, h, w = shape
    s = 1.5 / (n * h * w * c)
    closed = (ref_klc <= cs["floor"]).view(1, c, 1, 1).expand(shape)
    assert (cs["gmu"][closed] == 0).all() and (cs["glv"][closed] == 0).all(), "a closed gate passed a gradient"
    outside = cs["lv"].abs() > 10
    assert outside.any() and (cs["glv"][outside] == 0).all(), "logvar outside the clamp passed a gradient"
    assert (cs["glv"][(cs["lv"].abs() == 10) & ~closed] != 0).all()
    err = (cs["gmu"].double() - gmu64).abs()
    assert (err <= 4 * U * gmu64.abs() + 1e-300).all(), f"gmu: {(err / (4 * U * gmu64.abs() + 1e-300)).max().item():.3f}"
    lc = torch.clamp(cs["lv"].double(), -10, 10)
    tol = 4 * U * (glv64.abs() + s * torch.exp(lc)) + 1e-300          # 1 - exp(l) cancels near l = 0: absolute in the two parts
    err = (cs["glv"].double() - glv64).abs()
    assert (err <= tol).all(), f"glv: {(err / tol).max().item():.3f}"
    assert (gmu64[~closed] != 0).any()
    # pad lanes of the physical gradient buffers
    p = pkg.ops.pitch(c)
    if p != c:
        for g in (cs["gmu_raw"], cs["glv_raw"]):
            if pkg.ops.can_alias(g):              # (the C-ABI tests below look at the pad lanes of every buffer they hand in)
                assert (pkg.ops.phys_of(g)[..., c:] == 0).all(), "pad lanes of the gradient are not zero"


def _direct(pkg, device, mu, lv, c, floor, gout=1.0, stream=None, fill=float("nan")):
    """The C entries on physical (rows, cp) buffers -> (out3, klc, gmu, glv), outputs pre-filled so unwritten words show."""
    lib = pkg._native.lib()
    rows, cp = mu.shape
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out3 = torch.full((3,), fill, device=device)
    klc = torch.full((c,), fill, device=device)
    gmu, glv = torch.full_like(mu, fill), torch.full_like(lv, fill)
    ws = torch.empty(lib.vcg_kl_fb_workspace(rows, cp) // 4 + 4, device=device)
    g = torch.tensor([gout], device=device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream)
    pkg._native.check(lib.vcg_kl_fb_fwd(P(mu), P(lv), P(out3), P(klc), rows, c, cp, floor, P(ws), ws.numel() * 4, st), "vcg_kl_fb_fwd")
    pkg._native.check(lib.vcg_kl_fb_bwd(P(mu), P(lv), P(g), P(klc), P(gmu), P(glv), rows, c, cp, floor, st), "vcg_kl_fb_bwd")
    return out3, klc, gmu, glv, ws


def _rows(device, rows, cp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((rows, cp), generator=g).to(device), (torch.randn((rows, cp), generator=g) * 0.5).to(device)


def test_an_exact_tie_is_closed(pkg, device):
    mu, lv = _rows(device, 40, 8, 1)
    mu[:, 2], lv[:, 2] = 1.0, 0.0                 # k = -0.5 (1 + 0 - 1 - 1) = 0.5 for every element: KL_2 = 0.5 exactly
    out3, klc, gmu, glv, _ = _direct(pkg, device, mu, lv, 8, 0.5)
    torch.cuda.synchronize()
    assert klc[2].item() == 0.5
    assert (gmu[:, 2] == 0).all() and (glv[:, 2] == 0).all()
    others = torch.cat([klc[:2], klc[3:]]).double()
    want = (torch.clamp(others, min=0.5).sum().item() + 0.5) / 8
    assert abs(out3[0].item() - want) <= 2 * U * want
    assert out3[2].item() == int((others > 0.5).sum())


def test_a_floor_above_every_channel(pkg, device):
    mu, lv = _rows(device, 33, 12, 2)
    out3, klc, gmu, glv, _ = _direct(pkg, device, mu, lv, 10, 50.0)
    torch.cuda.synchronize()
    assert (klc < 50).all() and out3[0].item() == 50.0 and out3[2].item() == 0
    assert (gmu == 0).all() and (glv == 0).all()


def test_a_tiny_floor_gives_the_plain_gradient(pkg, device):
    lib = pkg._native.lib()
    mu, lv = _rows(device, 257, 64, 3)
    lv[5, 7], lv[9, 1] = 11.0, -10.5
    out3, klc, gmu, glv, _ = _direct(pkg, device, mu, lv, 64, 1e-30, gout=0.7)
    assert (klc > 1e-30).all() and out3[2].item() == 64
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    g = torch.tensor([0.7], device=device)
    pmu, plv = torch.empty_like(mu), torch.empty_like(lv)
    pkg._native.check(lib.vcg_kl_bwd(P(mu), P(lv), P(g), P(pmu), P(plv), mu.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                      "vcg_kl_bwd")
    torch.cuda.synchronize()
    assert ((gmu.double() - pmu.double()).abs() <= 2 * U * pmu.double().abs()).all()
    s = 0.7 / mu.numel()
    tol = 2 * U * (plv.double().abs() + s * torch.exp(torch.clamp(lv.double(), -10, 10)))
    assert ((glv.double() - plv.double()).abs() <= tol).all()
    assert glv[5, 7].item() == 0 and glv[9, 1].item() == 0
    assert abs(out3[0].item() - out3[1].item()) <= U * abs(out3[1].item())


def test_a_nan_channel_stays_open_and_reaches_the_loss(pkg, device):
    mu, lv = _rows(device, 20, 8, 4)
    mu[3, 5] = float("nan")
    out3, klc, gmu, glv, _ = _direct(pkg, device, mu, lv, 8, 0.4, fill=0.0)
    torch.cuda.synchronize()
    assert math.isnan(klc[5].item()) and math.isnan(out3[0].item()) and math.isnan(out3[1].item())
    assert not torch.isnan(torch.cat([klc[:5], klc[6:]])).any()
    keep = torch.ones(20, dtype=torch.bool)
    keep[3] = False
    assert (gmu[keep, 5] != 0).all() and math.isnan(gmu[3, 5].item()), "the NaN channel's gradient was gated"
    assert out3[2].item() == 1 + int((torch.cat([klc[:5], klc[6:]]) > 0.4).sum())


def test_same_input_same_bits_and_side_stream(pkg, device):
    mu, lv = _rows(device, 1031, 64, 5)
    first = _direct(pkg, device, mu, lv, 62, 0.3, gout=1.25)
    second = _direct(pkg, device, mu, lv, 62, 0.3, gout=1.25)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _direct(pkg, device, mu, lv, 62, 0.3, gout=1.25, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for name, a, b, c in zip(("out3", "klc", "gmu", "glv"), first, second, third):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two runs differ"
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), f"{name}: the side stream differs"
    assert (first[2][:, 62:] == 0).all() and (first[3][:, 62:] == 0).all()       # pad lanes, written as zeros over the NaN fill


# ------------------------------------------------------------------ routes of the autograd Function
def test_two_d_input(pkg, device):
    g = torch.Generator().manual_seed(6)
    mu, lv = torch.randn((37, 6), generator=g) * torch.tensor([0.3, 2.0, 0.3, 2.0, 0.3, 2.0]), torch.randn((37, 6), generator=g) * 0.5
    floor = median_floor(reference(mu, lv, 0.0)[3])
    loss64, plain64, active64, klc64, gmu64, glv64, absum = reference(mu, lv, floor)
    bound = channel_bound((37, 6, 1, 1), klc64, absum)
    assert_margin(klc64, floor, bound)
    mud, lvd = mu.to(device).requires_grad_(True), lv.to(device).requires_grad_(True)
    loss, plain, active = pkg.ops.kl_free_bits(mud, lvd, floor)
    assert not plain.requires_grad and not active.requires_grad and loss.requires_grad
    loss.backward()
    assert abs(loss.item() - loss64) <= bound.mean().item() + U * loss64 and active.item() == active64
    assert mud.grad.shape == (37, 6) and lvd.grad.shape == (37, 6)
    assert ((mud.grad.cpu().double() - gmu64).abs() <= 4 * U * gmu64.abs()).all()
    s = 1.0 / mu.numel()
    assert ((lvd.grad.cpu().double() - glv64).abs() <= 4 * U * (glv64.abs() + s * torch.exp(lv.double()))).all()


def test_foreign_layout_and_partial_gradients(pkg, device):
    """A plain NCHW latent (copied to the networks' layout) gives the bits of the same values handed over in that layout; with
    only mu or only logvar requiring a gradient the other comes back as None and the one computed keeps its bits."""
    cs = case(pkg, device, (3, 6, 2, 3))
    mu, lv, floor = cs["mu"], cs["lv"], cs["floor"]

    def run(need_mu, need_lv, foreign):
        a, b = (mu.to(device), lv.to(device)) if foreign else (to_dev(pkg, mu, device), to_dev(pkg, lv, device))
        a.requires_grad_(need_mu)
        b.requires_grad_(need_lv)
        loss, _, _ = pkg.ops.kl_free_bits(a, b, floor)
        (loss * 1.5).backward()
        return loss.item(), None if a.grad is None else nchw(a.grad), None if b.grad is None else nchw(b.grad)

    both = run(True, True, True)
    assert both[0] == cs["loss"] and torch.equal(both[1], cs["gmu"]) and torch.equal(both[2], cs["glv"])
    only_mu, only_lv = run(True, False, False), run(False, True, True)
    assert only_mu[2] is None and torch.equal(only_mu[1], cs["gmu"])
    assert only_lv[1] is None and torch.equal(only_lv[2], cs["glv"])


def test_expanded_gradient_and_second_differentiation(pkg, device):
    cs = case(pkg, device, (2, 64, 4, 4))
    mud, lvd = cs["mud"].detach().clone().requires_grad_(True), cs["lvd"].detach().clone().requires_grad_(True)
    loss, _, _ = pkg.ops.kl_free_bits(mud, lvd, cs["floor"])
    # the gradient of loss arrives as a stride-0 expansion's reduction and as an element of a larger tensor
    loss.expand(3).sum().backward(retain_graph=True)
    three = nchw(mud.grad)
    mud.grad = None
    scale = torch.tensor([9.0, 3.0, 9.0], device=device)
    loss.backward(scale[1], retain_graph=True)
    assert torch.equal(nchw(mud.grad), three)
    assert ((three.double() - 2 * cs["gmu"].double()).abs() <= 4 * U * three.double().abs()).all()      # 3 against the case's 1.5
    # a second differentiation: d/dw of d(w loss)/dmu runs through the Function's backward a second time
    w = torch.tensor(2.0, device=device, requires_grad=True)
    (gmu,) = torch.autograd.grad(loss * w, mud, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice a function that was marked with @once_differentiable"):
        gmu.sum().backward()


def test_bad_calls_are_refused(pkg, device):
    mu = torch.zeros((2, 8, 2, 2), device=device)
    for floor in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="floor"):
            pkg.ops.kl_free_bits(mu, mu, floor)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        pkg.ops.kl_free_bits(mu, mu[:, :4], 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.ops.kl_free_bits(mu.cpu(), mu.cpu(), 0.1)
    with pytest.raises(RuntimeError, match="latent"):
        pkg.ops.kl_free_bits(mu[0], mu[0], 0.1)
