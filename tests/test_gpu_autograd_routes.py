"""The autograd layer of ops.py on the routes Networks.py never takes: inputs the package did not make, gradients that arrive in
another layout, subsets of inputs that need a gradient, and graphs differentiated twice.

References: the same graph from plain torch ops in float64 on the device (the conv block through `test_custom_ops.torch_block`,
the losses through the float64 restatements of the per-loss tests), parameter gradients from the float64 parameters' `.grad`
after the same sequence of backward calls (the package accumulates into `.grad` and hands autograd None).  Two routes that run
the same kernels on the same values must agree BITWISE (`torch.equal`: the layout conversions are exact); a comparison with
float64 uses conftest.assert_close at its defaults (relative L2 1e-4, max 1e-3: the bound test_conv_blocks_match_oracle applies to
the same kernels), and a bias gradient that is analytically zero under an InstanceNorm follows that test's rule.

The out-of-bounds alias (x4[:, 1:4]) never comes here: tests/test_layout_host.py is its check."""
import pytest
import torch
import torch.nn.functional as F

from conftest import SEED, assert_close, max_rel, rel_l2
from test_custom_ops import torch_block
from test_gpu_freq_loss import freq_loss_ref
from test_gpu_grad_loss import grad_loss_ref
from test_gpu_ssim_loss import ssim_loss_ref

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def data(pkg, device, shape, key, scale=1.0):
    return (torch.from_numpy(pkg.synth.normal(tuple(shape), SEED, "routes/" + key)) * scale).to(device)


def nchw(ops, t):
    """A plain contiguous NCHW copy of t (a logical nhwc view or anything else)."""
    return ops.to_nchw_contiguous(t.detach())


class Block:
    """One conv block: its ConvSpec, fp32 parameters for ops.conv_block and float64 twins for `torch_block`."""

    def __init__(self, pkg, device, key, cin, cout, k, stride=1, pad=1, ups=1, epi=0, norm=False, post=0, shuffle=False, reflect=True):
        self.ops = pkg.ops
        self.geom = (stride, pad, ups, epi, norm, post, shuffle, reflect)
        self.spec = pkg.ops.ConvSpec(cin, cout, k, stride, pad, reflect, ups, epi, norm, post, shuffle)
        w0 = data(pkg, device, (cout, cin, k, k), key + "/w", (2.0 / (cin * k * k)) ** 0.5)
        b0 = data(pkg, device, (cout,), key + "/b", 0.1)
        self.w, self.b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
        self.w64, self.b64 = w0.double().requires_grad_(True), b0.double().requires_grad_(True)
        self.cancelled_bias = norm and epi == 0

    def __call__(self, x, residual=None, defer=False):
        return self.ops.conv_block(x, self.w, self.b, self.spec, residual=residual, defer=defer)

    def ref(self, x64, res64=None):
        return torch_block(x64, self.w64, self.b64, res64, *self.geom)

    def zero(self):
        self.w.grad = self.b.grad = None
        self.w64.grad = self.b64.grad = None

    def grads(self):
        return [None if p.grad is None else p.grad.clone() for p in (self.w, self.b)]

    def check_grads(self, what, out_scale=1.0, weight=True, bias=True):
        if weight:
            assert_close(self.w.grad, self.w64.grad, what + " dweight")
        if bias:
            ref = self.b64.grad
            if self.cancelled_bias:
                # InstanceNorm directly on conv + bias: analytically zero, the buffer (if there is one) stays at its zeros
                assert ref.abs().max().item() < 1e-4 * max(1.0, out_scale)
                assert self.b.grad is None or self.b.grad.abs().max().item() < 1e-2
            else:
                assert_close(self.b.grad, ref, what + " dbias")


def leaf(ops, x0):
    """x0 (NCHW values) as a leaf in the package's layout, and its float64 twin."""
    return ops.to_nhwc(x0).requires_grad_(True), x0.double().requires_grad_(True)


def same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(a, b), f"{what}: the two routes differ in {(a != b).sum().item()} of {a.numel()} values"


# ------------------------------------------------------------------ B.1 foreign inputs
def rgb_of_rgba(pkg, device, shape, key, alpha=7.0):
    """x4[:, :3] of a channels-last RGBA tensor with alpha = 7 (the target of a pair: 2, or the two alphas would cancel in a
    difference): the strides of the package's pitch-4 RGB image, alpha in the pad lane."""
    n, _, h, w = shape
    x4 = torch.empty((n, 4, h, w), device=device).to(memory_format=torch.channels_last)
    x4[:, :3] = data(pkg, device, shape, key)
    x4[:, 3] = alpha
    v = x4[:, :3]
    assert pkg.ops.is_nhwc_view(v)                          # (that it is not aliased: tests/test_layout_host.py, and the values below)
    return v


def _loss_entry(name):
    return {
        "l1_loss": lambda ops, a, b: ops.l1_loss(a, b),
        "ssim_loss": lambda ops, a, b: ops.ssim_loss(a, b),
        "grad_match_loss": lambda ops, a, b: ops.grad_match_loss(a, b, 3),
        "freq_loss": lambda ops, a, b: ops.freq_loss(a, b, 1.0),
    }[name]


@pytest.mark.parametrize("entry", ["l1_loss", "ssim_loss", "grad_match_loss", "freq_loss"])
def test_foreign_rgb_slice_is_copied_by_the_losses(entry, pkg, device):
    """Outcome for l1_loss, ssim_loss, grad_match_loss and freq_loss: the slice is COPIED (pad lanes zeroed), on both arguments;
    value and gradient are bitwise those of ops.to_nhwc(x4[:, :3].contiguous())."""
    ops, shape = pkg.ops, (2, 3, 16, 12)
    fa, fb = rgb_of_rgba(pkg, device, shape, entry + "/a"), rgb_of_rgba(pkg, device, shape, entry + "/b", alpha=2.0)
    f = _loss_entry(entry)
    xf = fa.detach().requires_grad_(True)
    assert xf.stride() == fa.stride()
    vf = f(ops, xf, fb)
    vf.backward()
    xo = ops.to_nhwc(fa.contiguous()).requires_grad_(True)
    vo = f(ops, xo, ops.to_nhwc(fb.contiguous()))
    vo.backward()
    same(vf.detach(), vo.detach(), entry + " value")
    same(xf.grad.contiguous(), nchw(ops, xo.grad), entry + " gradient")
    # ... and the value is the float64 one of the three colour channels alone
    a64, b64 = fa.double().contiguous().cpu(), fb.double().contiguous().cpu()       # the restatements are host code
    ref = {"l1_loss": lambda: (a64 - b64).abs().mean(), "ssim_loss": lambda: ssim_loss_ref(a64, b64),
           "grad_match_loss": lambda: grad_loss_ref(a64, b64, 3), "freq_loss": lambda: freq_loss_ref(a64, b64, 1.0)}[entry]()
    assert_close(vf.detach().reshape(1), ref.reshape(1), entry + " against float64")


def test_foreign_rgb_slice_is_copied_by_image_metrics(pkg, device):
    """Outcome for image_metrics: COPIED; bitwise the metrics of the converted copies."""
    ops, shape = pkg.ops, (2, 3, 12, 12)
    fa, fb = rgb_of_rgba(pkg, device, shape, "metrics/a"), rgb_of_rgba(pkg, device, shape, "metrics/b", alpha=2.0)
    fa.mul_(0.25).add_(0.5)
    fb.mul_(0.25).add_(0.5)
    got = ops.image_metrics(fa, fb)
    want = ops.image_metrics(ops.to_nhwc(fa.contiguous()), ops.to_nhwc(fb.contiguous()))
    same(got, want, "image_metrics")
    l1 = (fa.double().clamp(0, 1) - fb.double()).abs().mean(dim=(1, 2, 3))
    assert_close(got[:, 0], l1, "image_metrics l1 against float64")


def test_foreign_rgb_slice_is_copied_by_the_conv_block(pkg, device):
    """Outcome for conv_block (a CaSb(3, 64, 7) stem): COPIED; output, input gradient and parameter gradients bitwise those of
    the converted copy (alpha = 7 in the pad lane would move the operand maximum the fp16 split scales by)."""
    ops = pkg.ops
    blk = Block(pkg, device, "stem", 3, 64, 7, 1, 3, 1, ops.ACT_NONE, True, ops.ACT_RELU)
    fx = rgb_of_rgba(pkg, device, (1, 3, 16, 12), "stem/x")
    g0 = data(pkg, device, (1, 64, 16, 12), "stem/g")
    runs = []
    for x in (fx.detach().requires_grad_(True), ops.to_nhwc(fx.contiguous()).requires_grad_(True)):
        blk.zero()
        y = blk(x)
        y.backward(ops.to_nhwc(g0))
        runs.append((nchw(ops, y), nchw(ops, x.grad), *blk.grads()))
    for a, b, what in zip(runs[0], runs[1], ("y", "dx", "dweight", "dbias")):
        same(a, b, "stem " + what)
    x64 = fx.double().contiguous().requires_grad_(True)
    y64 = blk.ref(x64)
    y64.backward(g0.double())
    assert_close(runs[0][0], y64.detach(), "stem y against float64")
    assert_close(runs[0][1], x64.grad, "stem dx against float64")
    blk.check_grads("stem", y64.detach().abs().max().item())


def test_batch_one_channels_last_input_through_a_1x1_conv(pkg, device):
    """A (1, 8, 1, 5) channels-last tensor (pitch == C: no pad lanes; torch chooses the strides of its size-1 dimensions) through
    a zero-padded 1 x 1 convolution: aliased or copied, bitwise what the to_nhwc route gives."""
    ops = pkg.ops
    blk = Block(pkg, device, "one", 8, 8, 1, 1, 0, reflect=False)
    x0 = data(pkg, device, (1, 8, 1, 5), "one/x")
    g0 = data(pkg, device, (1, 8, 1, 5), "one/g")
    runs = []
    for x in (x0.to(memory_format=torch.channels_last).requires_grad_(True), ops.to_nhwc(x0).requires_grad_(True)):
        blk.zero()
        y = blk(x)
        y.backward(ops.to_nhwc(g0))
        runs.append((nchw(ops, y), nchw(ops, x.grad), *blk.grads()))
    for a, b, what in zip(runs[0], runs[1], ("y", "dx", "dweight", "dbias")):
        same(a, b, "1x1 " + what)
    x64 = x0.double().requires_grad_(True)
    y64 = F.conv2d(x64, blk.w64, blk.b64)
    y64.backward(g0.double())
    assert_close(runs[0][0], y64.detach(), "1x1 y")
    assert_close(runs[0][1], x64.grad, "1x1 dx")
    blk.check_grads("1x1")


# ------------------------------------------------------------------ B.2 gradient layouts
def _route_cases(pkg, device):
    ops = pkg.ops
    R, N = ops.ACT_RELU, ops.ACT_NONE

    def block_case(key, xshape, *spec, residual=False, pre=None):
        blk = Block(pkg, device, key, *spec)
        x0 = data(pkg, device, xshape, key + "/x")

        def build():
            blk.zero()
            x = ops.to_nhwc(x0).requires_grad_(True)
            h = pre(x) if pre is not None else x
            return blk(h, residual=h if residual else None), [x], [blk.w, blk.b]
        return build

    def shuffle_case():
        x0 = data(pkg, device, (2, 16, 5, 7), "ps/x")

        def build():
            x = ops.to_nhwc(x0).requires_grad_(True)
            return ops.pixel_shuffle(x), [x], []
        return build

    def pair_case():
        a, b = torch.nn.Conv2d(64, 8, 1).to(device), torch.nn.Conv2d(64, 8, 1).to(device)
        with torch.no_grad():
            for i, p in enumerate((a.weight, a.bias, b.weight, b.bias)):
                p.copy_(data(pkg, device, p.shape, f"pair/{i}", 0.1))
        pair = ops.FusedConvPair(a, b, ops.ConvSpec(64, 16, 1, 1, 0, False, 1))
        x0 = data(pkg, device, (2, 64, 4, 4), "pair/x")
        params = [a.weight, a.bias, b.weight, b.bias]

        def build():
            for p in params:
                p.grad = None
            x = ops.to_nhwc(x0).requires_grad_(True)
            return ops.conv_pair(x, pair)[0], [x], params
        return build

    def reparam_case():
        mu0, lv0, eps = (data(pkg, device, (2, 6, 3, 5), "rp/" + k) for k in ("mu", "lv", "eps"))

        def build():
            mu, lv = ops.to_nhwc(mu0).requires_grad_(True), ops.to_nhwc(lv0 * 8.0).requires_grad_(True)
            return ops.reparameterize(mu, lv, ops.to_nhwc(eps))[0], [mu, lv], []
        return build

    def to_nhwc_case():
        x0 = data(pkg, device, (2, 3, 5, 7), "tn/x")

        def build():
            x = x0.clone().requires_grad_(True)
            return ops.to_nhwc(x), [x], []
        return build

    return {
        "S 8->8": block_case("rS", (2, 8, 6, 10), 8, 8, 3),
        "D 8->8": block_case("rD", (3, 8, 4, 4), 32, 8, 3, 1, 1, 2, R, True),
        "U 128->64 shuffled store": block_case("rU", (2, 128, 8, 8), 32, 64, 3, 1, 1, 1, R, True, N, True, pre=ops.pixel_shuffle),
        "R 16 residual": block_case("rR", (1, 16, 3, 5), 16, 16, 3, 1, 1, 1, N, True, residual=True),
        "head 64->3 k7": block_case("rH", (1, 64, 24, 16), 64, 3, 7, 1, 3, 1, ops.ACT_TANH, False),
        "pixel_shuffle": shuffle_case(),
        "conv_pair": pair_case(),
        "reparameterize latent 6": reparam_case(),
        "to_nhwc": to_nhwc_case(),
    }


ROUTE_CASES = ["S 8->8", "D 8->8", "U 128->64 shuffled store", "R 16 residual", "head 64->3 k7", "pixel_shuffle", "conv_pair",
               "reparameterize latent 6", "to_nhwc"]


@pytest.mark.parametrize("case", ROUTE_CASES)
def test_gradient_layouts_give_the_same_bits(case, pkg, device):
    """The same gradient values arriving as an NHWC view, as a plain NCHW tensor and (all ones) as the stride-0 expansion of
    y.sum().backward(): every input gradient and every .grad buffer bitwise equal.  (conv_pair runs at latent 8: the fused pair
    refuses latent 6 — tests/test_layout_host.py — where the models run the two convolutions separately.)"""
    ops = pkg.ops
    build = _route_cases(pkg, device)[case]

    def run(send):
        y, leaves, params = build()
        send(y)
        got = []
        for t in leaves:
            assert t.grad is not None and torch.isfinite(t.grad).all()
            got.append((t.grad * 1.0).contiguous())          # usable by a torch op, whatever layout it came back in
        return got + [None if p.grad is None else p.grad.clone() for p in params]

    y, _, _ = build()
    g0 = data(pkg, device, tuple(y.shape), case + "/g")
    ones = torch.ones_like(g0)
    as_view = run(lambda y: y.backward(ops.to_nhwc(g0)))
    as_nchw = run(lambda y: y.backward(g0))
    for i, (a, b) in enumerate(zip(as_view, as_nchw)):
        same(a, b, f"{case}: NHWC view vs NCHW gradient, result {i}")
    ones_view = run(lambda y: y.backward(ops.to_nhwc(ones)))
    expanded = run(lambda y: y.sum().backward())
    for i, (a, b) in enumerate(zip(ones_view, expanded)):
        same(a, b, f"{case}: NHWC view of ones vs y.sum().backward(), result {i}")


def _scalar_losses(pkg, device):
    ops = pkg.ops
    a0, b0 = data(pkg, device, (2, 3, 16, 32), "sl/a", 0.25) + 0.5, data(pkg, device, (2, 3, 16, 32), "sl/b", 0.25) + 0.5
    mu0, lv0 = data(pkg, device, (2, 6, 3, 5), "sl/mu"), data(pkg, device, (2, 6, 3, 5), "sl/lv")
    loss = pkg.Losses.SlicedWassersteinLoss(levels=1, seed=3)
    plan = ops.SwdPlan(loss.offsets(2, 16, 32, 1), loss.directions(device, 1))
    b = ops.to_nhwc(b0)
    return {
        "l1": ([a0], lambda a: ops.l1_loss(a, b)),
        "ssim": ([a0], lambda a: ops.ssim_loss(a, b)),
        "grad": ([a0], lambda a: ops.grad_match_loss(a, b, 2)),
        "freq": ([a0], lambda a: ops.freq_loss(a, b, 0.5)),
        "swd": ([a0], lambda a: ops.swd_loss(a, b, 1, plan)),
        "kl": ([mu0, lv0], lambda m, l: ops.kl_loss(m, l)),
        "mse_const": ([mu0], lambda d: ops.mse_const(d, 1.0)[0]),
        "weighted_sum": ([a0], lambda a: ops.weighted_sum([ops.l1_loss(a, b), ops.ssim_loss(a, b)], [0.5, 3.0])),
    }


@pytest.mark.parametrize("name", ["l1", "ssim", "grad", "freq", "swd", "kl", "mse_const", "weighted_sum"])
def test_scalar_losses_take_their_gradient_scale_either_way(name, pkg, device):
    """(2 * loss).backward() and loss.backward(torch.tensor(2.)) hand the same 2.0 over: bitwise equal gradients."""
    ops = pkg.ops
    inputs, f = _scalar_losses(pkg, device)[name]

    def run(send):
        xs = [ops.to_nhwc(x0).requires_grad_(True) for x0 in inputs]
        send(f(*xs))
        return [nchw(ops, x.grad) for x in xs]

    scaled = run(lambda loss: (2 * loss).backward())
    given = run(lambda loss: loss.backward(torch.tensor(2.0, device=device)))
    for a, b in zip(scaled, given):
        assert a.abs().max().item() > 0
        same(a, b, name)


# ------------------------------------------------------------------ B.3 which inputs need a gradient
def _l1_pairs(pkg, device):
    a4, b4 = data(pkg, device, (2, 3, 7, 5), "l1/a"), data(pkg, device, (2, 3, 7, 5), "l1/b")
    a2, b2 = data(pkg, device, (5, 6), "l1/a2"), data(pkg, device, (5, 6), "l1/b2")
    return {"4d": (a4, b4, True), "2d-transposed": (a2, b2, False)}


@pytest.mark.parametrize("mode", ["a", "b", "both", "self"])
@pytest.mark.parametrize("kind", ["4d", "2d-transposed"])
def test_l1_loss_gradient_subsets(kind, mode, pkg, device):
    ops = pkg.ops
    a0, b0, four_d = _l1_pairs(pkg, device)[kind]

    def mk(t, grad):
        t = ops.to_nhwc(t) if four_d else t.clone()
        t = t.requires_grad_(grad)
        return t, (t if four_d else t.t())                    # a (6, 5) transposed view of the (5, 6) leaf

    (a, av), (b, bv) = mk(a0, mode != "b"), mk(b0, mode in ("b", "both"))
    a64 = a0.double().requires_grad_(mode != "b")
    b64 = b0.double().requires_grad_(mode in ("b", "both"))
    if mode == "self":
        loss, ref = ops.l1_loss(av, av.detach()), (a64 - a64.detach()).abs().mean()
    else:
        loss, ref = ops.l1_loss(av, bv), (a64 - b64).abs().mean()
    (3.0 * loss).backward()
    (3.0 * ref).backward()
    if mode == "self":
        assert loss.item() == 0.0 and a.grad.abs().max().item() == 0.0     # sign(0) = 0
        return
    assert_close(loss.detach().reshape(1), ref.detach().reshape(1), "l1 value")
    for t, t64, want in ((a, a64, mode != "b"), (b, b64, mode in ("b", "both"))):
        if want:
            assert_close(nchw(ops, t.grad) if four_d else t.grad, t64.grad, f"l1 {kind} {mode}")
        else:
            assert t.grad is None
    if mode == "both":
        ga, gb = (nchw(ops, t.grad) if four_d else t.grad for t in (a, b))
        same(gb, -ga, "gb = -ga")


@pytest.mark.parametrize("shape", [(2, 6, 3, 5), (4, 6)], ids=["4d-latent6", "2d"])
def test_kl_loss_against_float64(shape, pkg, oracle, device):
    """The mean runs over the logical values: latent 6 lives at pitch 8, and the pad lanes must not enter the count."""
    ops = pkg.ops
    mu0, lv0 = data(pkg, device, shape, "kl/mu"), data(pkg, device, shape, "kl/lv", 4.0)
    lv0.view(-1)[:4] = torch.tensor([10.0, -10.0, 12.0, -12.0], device=device)                # at and beyond the clamp
    conv = ops.to_nhwc if len(shape) == 4 else (lambda t: t.clone())
    mu, lv = conv(mu0).requires_grad_(True), conv(lv0).requires_grad_(True)
    loss = ops.kl_loss(mu, lv)
    loss.backward()
    mu64, lv64 = mu0.double().requires_grad_(True), lv0.double().requires_grad_(True)
    ref = oracle.kl_loss(mu64, lv64)
    ref.backward()
    back = (lambda t: nchw(ops, t)) if len(shape) == 4 else (lambda t: t)
    assert_close(loss.detach().reshape(1), ref.detach().reshape(1), "kl value")
    assert_close(back(mu.grad), mu64.grad, "kl dmu")
    assert_close(back(lv.grad), lv64.grad, "kl dlogvar")


def test_mse_const_forms(pkg, device):
    ops = pkg.ops
    d0 = data(pkg, device, (7, 5), "mse/d")
    # only the mean is used downstream: it is not differentiable, nothing reaches d
    d = d0.clone().requires_grad_(True)
    loss, mean = ops.mse_const(d, 1.0)
    assert not mean.requires_grad and mean.grad_fn is None and loss.requires_grad
    assert (mean * 2.0).grad_fn is None and d.grad is None                   # no graph behind it: no backward kernel can run
    assert_close(mean.reshape(1), d0.double().mean().reshape(1), "mean")
    # only the loss, of a contiguous and of a transposed d
    for view in (lambda t: t, lambda t: t.t()):
        d = d0.clone().requires_grad_(True)
        d64 = d0.double().requires_grad_(True)
        loss, _ = ops.mse_const(view(d), 1.0)
        (0.5 * loss).backward()
        ref = ((view(d64) - 1.0) ** 2).mean()
        (0.5 * ref).backward()
        assert_close(loss.detach().reshape(1), ref.detach().reshape(1), "mse value")
        assert_close(d.grad, d64.grad, "mse gradient")


@pytest.mark.parametrize("use", ["z", "logvar", "both"])
def test_reparameterize_gradient_subsets(use, pkg, device):
    """Latent 6 (pitch 8).  The unused output's gradient arrives as materialised NCHW zeros; the clamp passes the gradient on
    [-10, 10], edges included, and blocks it outside."""
    ops = pkg.ops
    shape = (2, 6, 3, 5)
    mu0, eps0 = data(pkg, device, shape, "rp3/mu"), data(pkg, device, shape, "rp3/eps")
    lv0 = data(pkg, device, shape, "rp3/lv", 6.0)
    lv0.view(-1)[:4] = torch.tensor([10.0, -10.0, 10.5, -10.5], device=device)
    gz, gl = data(pkg, device, shape, "rp3/gz"), data(pkg, device, shape, "rp3/gl")
    mu, lv = ops.to_nhwc(mu0).requires_grad_(True), ops.to_nhwc(lv0).requires_grad_(True)
    z, lvc = ops.reparameterize(mu, lv, ops.to_nhwc(eps0))
    mu64, lv64 = mu0.double().requires_grad_(True), lv0.double().requires_grad_(True)
    lvc64 = torch.clamp(lv64, -10, 10)
    z64 = mu64 + eps0.double() * torch.exp(0.5 * lvc64)
    loss = (z * gz).sum() if use == "z" else (lvc * gl).sum() if use == "logvar" else (z * gz).sum() + (lvc * gl).sum()
    ref = (z64 * gz.double()).sum() if use == "z" else (lvc64 * gl.double()).sum() if use == "logvar" else \
        (z64 * gz.double()).sum() + (lvc64 * gl.double()).sum()
    loss.backward()
    ref.backward()
    assert_close(nchw(ops, z), z64.detach(), "z")
    assert_close(nchw(ops, lvc), lvc64.detach(), "clamped logvar")
    if use == "logvar":
        assert mu.grad is None or mu.grad.abs().max().item() == 0.0
    else:
        assert_close(nchw(ops, mu.grad), mu64.grad, "dmu")
    glv = nchw(ops, lv.grad)
    assert_close(glv, lv64.grad, "dlogvar")
    flat = glv.view(-1)
    assert flat[2].item() == 0.0 and flat[3].item() == 0.0, "beyond the clamp the gradient is zero"
    if use != "z":
        assert flat[0].item() != 0.0 and flat[1].item() != 0.0, "at the clamp's edges the gradient passes (torch.clamp's subgradient)"


def _pair(pkg, device, key="cp"):
    ops = pkg.ops
    a, b = torch.nn.Conv2d(64, 8, 3).to(device), torch.nn.Conv2d(64, 8, 3).to(device)
    with torch.no_grad():
        for i, p in enumerate((a.weight, a.bias, b.weight, b.bias)):
            p.copy_(data(pkg, device, p.shape, f"{key}/{i}", 0.05))
    pair = ops.FusedConvPair(a, b, ops.ConvSpec(64, 16, 3, 1, 1, True, 1))
    twins = [p.detach().double().requires_grad_(True) for p in (a.weight, a.bias, b.weight, b.bias)]
    return a, b, pair, twins


def _pair_ref(x64, twins):
    xp = F.pad(x64, (1, 1, 1, 1), mode="reflect")
    return F.conv2d(xp, twins[0], twins[1]), F.conv2d(xp, twins[2], twins[3])


@pytest.mark.parametrize("use", ["mu", "logvar"])
def test_conv_pair_with_one_output_used(use, pkg, device):
    """The unused half reaches _ChanSplitFn.backward as materialised zeros: its member's gradient is zero, the other's and the
    input's match float64."""
    ops = pkg.ops
    a, b, pair, twins = _pair(pkg, device)
    x0, g0 = data(pkg, device, (2, 64, 4, 6), "cp/x"), data(pkg, device, (2, 8, 4, 6), "cp/g")
    x, x64 = leaf(ops, x0)
    out = ops.conv_pair(x, pair)[0 if use == "mu" else 1]
    (out * ops.to_nhwc(g0)).sum().backward()
    ref = _pair_ref(x64, twins)[0 if use == "mu" else 1]
    (ref * g0.double()).sum().backward()
    assert_close(nchw(ops, out), ref.detach(), "conv_pair " + use)
    assert_close(nchw(ops, x.grad), x64.grad, "conv_pair dx")
    used, idle = ((a, twins[:2]), (b, twins[2:])) if use == "mu" else ((b, twins[2:]), (a, twins[:2]))
    assert_close(used[0].weight.grad, used[1][0].grad, "used member dweight")
    assert_close(used[0].bias.grad, used[1][1].grad, "used member dbias")
    assert idle[0].weight.grad.abs().max().item() == 0.0 and idle[0].bias.grad.abs().max().item() == 0.0


def test_conv_pair_leaves_a_frozen_member_alone(pkg, device):
    """FusedConvPair fuses a frozen member with a trainable one (requires_grad is the OR): the backward must not write the
    frozen member's .grad — None stays None, a buffer keeps its bits — and must not keep its share of the scratch gradient for
    the day it trains again."""
    ops = pkg.ops
    a, b, pair, twins = _pair(pkg, device, "cpf")
    x0, g0 = data(pkg, device, (2, 64, 4, 6), "cpf/x"), data(pkg, device, (2, 8, 4, 6), "cpf/g")
    a.weight.requires_grad_(False)
    a.bias.requires_grad_(False)
    x, x64 = leaf(ops, x0)
    mu, lv = ops.conv_pair(x, pair)
    ((mu + lv) * ops.to_nhwc(g0)).sum().backward()
    r_mu, r_lv = _pair_ref(x64, twins)
    ((r_mu + r_lv) * g0.double()).sum().backward()
    assert a.weight.grad is None and a.bias.grad is None
    assert_close(b.weight.grad, twins[2].grad, "trainable member dweight")
    assert_close(b.bias.grad, twins[3].grad, "trainable member dbias")
    assert_close(nchw(ops, x.grad), x64.grad, "dx")
    # an existing buffer keeps its bits
    a.weight.grad = torch.full_like(a.weight, 0.25)
    x2 = ops.to_nhwc(x0).requires_grad_(True)
    mu, lv = ops.conv_pair(x2, pair)
    ((mu + lv) * ops.to_nhwc(g0)).sum().backward()
    assert torch.equal(a.weight.grad, torch.full_like(a.weight, 0.25))
    # thawed: its gradient is that of ONE backward, not of the three that ran meanwhile
    a.weight.requires_grad_(True)
    a.bias.requires_grad_(True)
    a.weight.grad = None
    x3 = ops.to_nhwc(x0).requires_grad_(True)
    mu, lv = ops.conv_pair(x3, pair)
    ((mu + lv) * ops.to_nhwc(g0)).sum().backward()
    assert_close(a.weight.grad, twins[0].grad, "thawed member dweight")
    assert_close(a.bias.grad, twins[1].grad, "thawed member dbias")


BIAS_PLACEMENTS = {"norm+epi": (3, 1, 1, 1, 1, True, 0), "norm only": (3, 1, 1, 1, 0, True, 1), "no norm": (3, 1, 1, 1, 2, False, 0)}


@pytest.mark.parametrize("placement", list(BIAS_PLACEMENTS))
def test_zero_padded_conv_block_against_float64(placement, pkg, device):
    """reflect=False: the reference is F.pad(mode="constant") in front of the same conv2d; output and every gradient."""
    ops = pkg.ops
    k, stride, pad, ups, epi, norm, post = BIAS_PLACEMENTS[placement]
    blk = Block(pkg, device, "zp/" + placement, 8, 12, k, stride, pad, ups, epi, norm, post, reflect=False)
    x0, g0 = data(pkg, device, (2, 8, 5, 7), "zp/x"), data(pkg, device, (2, 12, 5, 7), "zp/g")
    x, x64 = leaf(ops, x0)
    y, y64 = blk(x), blk.ref(x64)
    y.backward(ops.to_nhwc(g0))
    y64.backward(g0.double())
    assert_close(nchw(ops, y), y64.detach(), "y")
    assert_close(nchw(ops, x.grad), x64.grad, "dx")
    blk.check_grads("zero-padded " + placement, y64.detach().abs().max().item())


@pytest.mark.parametrize("mode", ["first layer", "weight frozen", "no_wgrad", "no_dgrad"])
@pytest.mark.parametrize("placement", list(BIAS_PLACEMENTS))
def test_conv_block_gradient_subsets(placement, mode, pkg, device):
    """The skipped gradient is None (or untouched), the others match float64; over the three places the backward takes the bias
    gradient from: the InstanceNorm backward (norm + epilogue activation), nowhere (norm alone: analytically zero) and the
    weight gradient's column sums (no norm)."""
    ops = pkg.ops
    k, stride, pad, ups, epi, norm, post = BIAS_PLACEMENTS[placement]
    blk = Block(pkg, device, "sub/" + placement, 8, 12, k, stride, pad, ups, epi, norm, post)
    x0, g0 = data(pkg, device, (2, 8, 5, 7), "sub/x"), data(pkg, device, (2, 12, 5, 7), "sub/g")
    x = ops.to_nhwc(x0).requires_grad_(mode != "first layer")
    x64 = x0.double().requires_grad_(mode != "first layer")
    if mode == "weight frozen":              # the bias stays trainable: its gradient must still come
        blk.w.requires_grad_(False)
        blk.w64.requires_grad_(False)
    y = blk(x)
    y64 = blk.ref(x64)
    if mode == "no_wgrad":
        with ops.no_wgrad([blk.w, blk.b]):
            y.backward(ops.to_nhwc(g0))
    elif mode == "no_dgrad":
        with ops.no_dgrad([blk.spec]):
            y.backward(ops.to_nhwc(g0))
    else:
        y.backward(ops.to_nhwc(g0))
    y64.backward(g0.double())
    scale = y64.detach().abs().max().item()
    assert_close(nchw(ops, y), y64.detach(), "y")
    if mode in ("first layer", "no_dgrad"):
        assert x.grad is None
    else:
        assert_close(nchw(ops, x.grad), x64.grad, "dx")
    if mode == "no_wgrad":
        assert blk.w.grad is None and blk.b.grad is None
    elif mode == "weight frozen":
        assert blk.w.grad is None
        blk.check_grads(f"{placement} {mode}", scale, weight=False)
    else:
        blk.check_grads(f"{placement} {mode}", scale)


@pytest.mark.parametrize("term", ["ssim", "grad", "freq", "swd"])
def test_image_terms_with_a_detached_generated_image(term, pkg, device):
    """With `generated` detached the term contributes a value and no gradient: a sum with a live L1 term differentiates to the L1
    gradient alone, bitwise.  A target that requires a gradient stays refused."""
    ops = pkg.ops
    a0, b0 = data(pkg, device, (2, 3, 16, 32), "it/a", 0.25) + 0.5, data(pkg, device, (2, 3, 16, 32), "it/b", 0.25) + 0.5
    loss = pkg.Losses.SlicedWassersteinLoss(levels=1, seed=3)
    plan = ops.SwdPlan(loss.offsets(2, 16, 32, 1), loss.directions(device, 1))
    f = {"ssim": lambda a, b: ops.ssim_loss(a, b), "grad": lambda a, b: ops.grad_match_loss(a, b, 2),
         "freq": lambda a, b: ops.freq_loss(a, b, 1.0), "swd": lambda a, b: ops.swd_loss(a, b, 1, plan)}[term]
    b = ops.to_nhwc(b0)
    a = ops.to_nhwc(a0).requires_grad_(True)
    l1 = ops.l1_loss(a, b)
    dead = f(a.detach(), b)
    assert not dead.requires_grad
    (l1 + dead).backward()
    a2 = ops.to_nhwc(a0).requires_grad_(True)
    ops.l1_loss(a2, b).backward()
    same(nchw(ops, a.grad), nchw(ops, a2.grad), term + ": the live term's gradient alone")
    # through weighted_sum, and with the dead term's input an intermediate that needs no gradient
    a3 = ops.to_nhwc(a0).requires_grad_(True)
    ops.weighted_sum([ops.l1_loss(a3, b), f(a3.detach(), b)], [1.0, 5.0]).backward()
    same(nchw(ops, a3.grad), nchw(ops, a2.grad), term + ": through weighted_sum")
    with pytest.raises(RuntimeError, match="the target must not require a gradient"):
        f(a, ops.to_nhwc(b0).requires_grad_(True))


WSUM_CASES = {"one": ([0], [1.5]), "same twice": ([0, 0], [0.5, 2.0]), "dead term": ([0, None, 1], [2.0, 3.0, 0.25]),
              "zero weight": ([0, 1], [0.0, 1.0]), "sixteen": (list(range(16)), [0.5 + 0.37 * i for i in range(16)])}


@pytest.mark.parametrize("case", list(WSUM_CASES))
def test_weighted_sum_against_float64(case, pkg, device):
    ops = pkg.ops
    idx, weights = WSUM_CASES[case]
    v0 = data(pkg, device, (16,), "ws/v")
    dead = torch.tensor(0.75, device=device)
    leaves = [v0[i].clone().requires_grad_(True) for i in range(16)]
    twins = [v0[i].double().clone().requires_grad_(True) for i in range(16)]
    out = ops.weighted_sum([dead if i is None else leaves[i] for i in idx], weights)
    ref = sum(w * (dead.double() if i is None else twins[i]) for i, w in zip(idx, weights))
    (2.0 * out).backward()
    (2.0 * ref).backward()
    assert_close(out.detach().reshape(1), ref.detach().reshape(1), "weighted_sum")
    for i in set(j for j in idx if j is not None):
        if twins[i].grad.item() == 0.0:
            assert leaves[i].grad.item() == 0.0
        else:
            assert_close(leaves[i].grad.reshape(1), twins[i].grad.reshape(1), f"weighted_sum d term {i}")
    for i in range(16):
        if i not in idx:
            assert leaves[i].grad is None


def _sn_setup(pkg, device):
    """The smallest legal map of test_sn_prepare's list: a 20 x 3 x 5 head."""
    C, KH, KW = 20, 3, 5
    w0 = data(pkg, device, (1, C, KH, KW), "sn/w", 0.05)
    v0 = F.normalize(data(pkg, device, (C * KH * KW,), "sn/v"), dim=0)
    x0 = data(pkg, device, (4, C, KH, KW), "sn/x")
    g0 = data(pkg, device, (4,), "sn/g")
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


@pytest.mark.parametrize("mode", ["all", "x detached", "weight frozen", "no_wgrad"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_fullmap_sn_conv_gradient_subsets(training, mode, pkg, device):
    ops = pkg.ops
    w0, u0, v0, b0, x0, g0 = _sn_setup(pkg, device)
    w, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    u, v = u0.clone(), v0.clone()
    w64, b64 = w0.double().requires_grad_(mode != "weight frozen"), b0.double().requires_grad_(True)
    if mode == "weight frozen":              # the bias stays trainable
        w.requires_grad_(False)
    x = ops.to_nhwc(x0).requires_grad_(mode != "x detached")
    x64 = x0.double().requires_grad_(mode != "x detached")
    out = ops.fullmap_sn_conv(x, w, b, u, v, training)
    ref = _sn_ref(x64, w64, b64, u0, v0, training)
    if mode == "no_wgrad":
        with ops.no_wgrad([w, b]):
            out.backward(g0)
    else:
        out.backward(g0)
    ref.backward(g0.double())
    assert_close(out.detach(), ref.detach(), "fullmap y")
    if training:
        assert not torch.equal(v, v0), "training mode advances v in place"
    else:
        assert torch.equal(v, v0) and torch.equal(u, u0)
    if mode == "x detached":
        assert x.grad is None
    else:
        assert_close(nchw(ops, x.grad), x64.grad, "fullmap dx")
    if mode == "no_wgrad":
        assert w.grad is None and b.grad is None
    elif mode == "weight frozen":
        assert w.grad is None
        assert_close(b.grad, b64.grad, "fullmap dbias under a frozen weight")
    else:
        assert_close(w.grad, w64.grad, "fullmap dweight")
        assert_close(b.grad, b64.grad, "fullmap dbias")


# ------------------------------------------------------------------ B.4 one graph, two traversals
def _chain(pkg, device):
    blk1 = Block(pkg, device, "ch/1", 256, 256, 3)
    blk2 = Block(pkg, device, "ch/2", 256, 64, 3)
    x0, g0 = data(pkg, device, (2, 256, 8, 8), "ch/x"), data(pkg, device, (2, 64, 8, 8), "ch/g")
    return blk1, blk2, x0, g0


def test_two_block_chain_differentiated_twice(pkg, device):
    """S(256 -> 256) -> S(256 -> 64) on 8 x 8 maps (Winograd layers that keep forward state for the weight gradient): the first
    backward consumes the kept state, the second recomputes it; .grad is the float64 .grad after two backwards."""
    ops = pkg.ops
    blk1, blk2, x0, g0 = _chain(pkg, device)
    x, x64 = leaf(ops, x0)
    y, y64 = blk2(blk1(x)), blk2.ref(blk1.ref(x64))
    for _ in range(2):
        y.backward(ops.to_nhwc(g0), retain_graph=True)
        y64.backward(g0.double(), retain_graph=True)
    assert_close(nchw(ops, y), y64.detach(), "chain y")
    assert_close(nchw(ops, x.grad), x64.grad, "chain dx after two backwards")
    blk1.check_grads("chain block 1, two backwards")
    blk2.check_grads("chain block 2, two backwards")


@pytest.mark.parametrize("order", ["no_wgrad first", "no_dgrad first"])
def test_two_block_chain_in_phase_order(order, pkg, device):
    """The models' alternation on one retained graph: a traversal under no_wgrad (data gradient only) and one under no_dgrad on
    the first spec (weight gradients only, nothing for x), in both orders."""
    ops = pkg.ops
    blk1, blk2, x0, g0 = _chain(pkg, device)
    x, x64 = leaf(ops, x0)
    y, y64 = blk2(blk1(x)), blk2.ref(blk1.ref(x64))
    params = [blk1.w, blk1.b, blk2.w, blk2.b]

    def data_only():
        with ops.no_wgrad(params):
            y.backward(ops.to_nhwc(g0), retain_graph=True)
        assert all(p.grad is None for p in params) or order == "no_dgrad first"

    def weights_only():
        before = None if x.grad is None else x.grad.clone()
        with ops.no_dgrad([blk1.spec]):
            y.backward(ops.to_nhwc(g0), retain_graph=True)
        assert (x.grad is None) if before is None else torch.equal(x.grad, before)

    for step in ((data_only, weights_only) if order == "no_wgrad first" else (weights_only, data_only)):
        step()
    y64.backward(g0.double())
    assert_close(nchw(ops, x.grad), x64.grad, "phase dx")
    blk1.check_grads("phase block 1")
    blk2.check_grads("phase block 2")


def test_deferred_hand_off_backward_once_then_refusal(pkg, device):
    """D(64, 128) hands its raw output and statistics to D(128, 256) (the geometry of
    test_deferred_instance_norm_equals_the_materialised_path).  The first backward matches float64 — the input gradient and both
    blocks' weight and bias gradients, at assert_close's defaults.  The consumer's weight gradient has then handed back the kept
    state a deferred input cannot be recomputed from: a second backward raises before it has accumulated anything, so every
    .grad keeps its bits."""
    ops = pkg.ops
    R = ops.ACT_RELU
    d1 = Block(pkg, device, "df/1", 256, 128, 3, 1, 1, 2, R, True)
    d2 = Block(pkg, device, "df/2", 512, 256, 3, 1, 1, 2, R, True)
    x0, g0 = data(pkg, device, (2, 64, 64, 64), "df/x"), data(pkg, device, (2, 256, 16, 16), "df/g")
    assert ops.consumer_takes_deferred(d2.spec, 2, 32, 32)
    x, x64 = leaf(ops, x0)
    h = d1(x, defer=True)
    assert getattr(h, "_vcg_lazy", None) is not None
    y = d2(h)
    y64 = d2.ref(d1.ref(x64))
    y.backward(ops.to_nhwc(g0), retain_graph=True)
    y64.backward(g0.double())
    params = (d1.w, d1.b, d2.w, d2.b)
    kept = [p.grad.clone() for p in params] + [nchw(ops, x.grad)]
    with pytest.raises(RuntimeError, match="needs the forward's kept state"):
        y.backward(ops.to_nhwc(g0))
    for p, before, what in zip(params, kept, ("producer weight", "producer bias", "consumer weight", "consumer bias")):
        assert torch.equal(p.grad, before), f"the refused traversal wrote the {what} gradient"
    assert torch.equal(nchw(ops, x.grad), kept[4]), "the refused traversal wrote the input gradient"
    for name, got, want in (("y", nchw(ops, y), y64.detach()), ("dx", kept[4], x64.grad),
                            ("producer dweight", d1.w.grad, d1.w64.grad), ("producer dbias", d1.b.grad, d1.b64.grad),
                            ("consumer dweight", d2.w.grad, d2.w64.grad), ("consumer dbias", d2.b.grad, d2.b64.grad)):
        print(f"deferred {name}: rel_l2 {rel_l2(got, want):.3e} max_rel {max_rel(got, want):.3e}")
    assert_close(nchw(ops, y), y64.detach(), "deferred y")
    assert_close(kept[4], x64.grad, "deferred dx")
    d1.check_grads("deferred producer")
    d2.check_grads("deferred consumer")


@pytest.mark.parametrize("mid", [3, 64])
def test_a_tensor_consumed_twice(mid, pkg, device):
    """y = block1(x) feeds two blocks: autograd sums two gradients that arrive as NHWC views (at 3 channels: pitch 4, and what
    torch allocates for the sum has no pad lanes of the package's) before block1's backward sees them.  (Tanh and LeakyReLU
    heads: a Sigmoid block with 3 output channels is refused by ConvSpec, tests/test_layout_host.py.)"""
    ops = pkg.ops
    b1 = Block(pkg, device, f"tw{mid}/1", 8, mid, 3)
    b2 = Block(pkg, device, f"tw{mid}/2", mid, 3, 3, 1, 1, 1, ops.ACT_TANH, False)
    b3 = Block(pkg, device, f"tw{mid}/3", mid, 3, 3, 1, 1, 1, ops.ACT_LEAKY, False)
    x0, t0 = data(pkg, device, (2, 8, 6, 10), "tw/x"), data(pkg, device, (2, 3, 6, 10), "tw/t", 0.3)
    x, x64 = leaf(ops, x0)
    t = ops.to_nhwc(t0)
    y = b1(x)
    loss = ops.l1_loss(b2(y), t) + ops.l1_loss(b3(y), t)
    y64 = b1.ref(x64)
    ref = (b2.ref(y64) - t0.double()).abs().mean() + (b3.ref(y64) - t0.double()).abs().mean()
    loss.backward()
    ref.backward()
    assert_close(loss.detach().reshape(1), ref.detach().reshape(1), "loss")
    assert_close(nchw(ops, x.grad), x64.grad, "dx")
    for i, b in enumerate((b1, b2, b3)):
        b.check_grads(f"block {i + 1}")


def test_fullmap_sn_conv_differentiated_twice(pkg, device):
    """Training mode: both traversals use the u, v (and the normalised weight) of their own forward; a forward in between, on
    a weight that has moved, advances the module's u, v in place and must not change the second traversal."""
    ops = pkg.ops
    w0, u0, v0, b0, x0, g0 = _sn_setup(pkg, device)
    w, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    u, v = u0.clone(), v0.clone()
    x, x64 = leaf(ops, x0)
    w64, b64 = w0.double().requires_grad_(True), b0.double().requires_grad_(True)
    out = ops.fullmap_sn_conv(x, w, b, u, v, True)
    ref = _sn_ref(x64, w64, b64, u0, v0, True)
    out.backward(g0, retain_graph=True)
    ref.backward(g0.double(), retain_graph=True)
    first = (nchw(ops, x.grad).clone(), w.grad.clone(), b.grad.clone())
    # a forward in between, after the weight has moved as an optimizer step moves it, advances the module's u, v in place (on
    # the unchanged weight a second power iteration of a one-output-channel map would reproduce them)
    v_then = v.clone()
    with torch.no_grad():
        w.add_(data(pkg, device, tuple(w.shape), "sn/w step", 0.05))
        ops.fullmap_sn_conv(ops.to_nhwc(x0), w, b, u, v, True)
    assert not torch.equal(v, v_then)
    out.backward(g0)
    ref.backward(g0.double())
    assert_close(nchw(ops, x.grad), x64.grad, "dx after two traversals")
    assert_close(w.grad, w64.grad, "dweight after two traversals")
    assert_close(b.grad, b64.grad, "dbias after two traversals")
    # the second traversal added what the first did: it saw the forward's u, v, not the advanced ones
    assert_close(nchw(ops, x.grad) - first[0], first[0], "the second traversal's dx")
    assert_close(w.grad - first[1], first[1], "the second traversal's dweight")
