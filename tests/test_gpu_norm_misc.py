"""The InstanceNorm, activation, layout, loss, reparameterisation and spectral-norm entry points of csrc/norm.hip and
csrc/misc.hip, called one by one through the C ABI and compared with torch in float64 on the device.

Every output is prefilled with NaN and followed by a guard band of sentinel words: an element the kernel does not write, or a
store past the end (the pixel-shuffled stores, gbias[c_log:]), fails the test.

Tolerances follow from fp32 rounding (U = 2^-24, the unit roundoff) of the operation as the kernel computes it:
  * elementwise formulas: a few U of the magnitudes of their own terms;
  * fp32 sums: the worst-case bound L * U * sum|terms|, with L the depth of the kernel's summation tree (its launch plan);
  * InstanceNorm forward: the statistics are double sums rounded once to fp32 (~U); the normalised value (t - mean) * rstd carries
    the rounding of mean and rstd, i.e. U * (|xhat| + rstd * |mean|);
  * InstanceNorm backward: dt = epi'(t) rstd (g' - s1 - xhat s2) carries U * rstd * (|g'| + |s1| + |xhat s2|) per operation
    (plus the error of xhat times s2, and times g'' for Tanh / Sigmoid).  Where the three terms cancel, the kernel's error must
    in addition be no worse than 4x PyTorch's own fp32 error against the same float64 reference.
At a ReLU / LeakyReLU kink the derivative is taken on the side the fp32 normalised value lies (what the kernel sees); the float64
reference differentiates the same piecewise function with that side fixed.
"""
import ctypes
import json
import math
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_gpu_fullsize import NORM_CASES

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = torch.tensor(1e-5, dtype=torch.float32).item()     # nn.InstanceNorm2d's eps as the C ABI receives it (a float)
NONE, RELU, LEAKY, TANH, SIGMOID = 0, 1, 2, 3, 4
ACTS = {NONE: "none", RELU: "relu", LEAKY: "leaky", TANH: "tanh", SIGMOID: "sigmoid"}
GUARD = 64
SENTINEL = 0x5EADBEEF
NAN = float("nan")


# ------------------------------------------------------------------ the InstanceNorm case list and its launch plan
def norm_plan(N, HW, C):
    """Python mirror of vcg_norm_plan (csrc/vcg_common.h)."""
    c4 = C // 4
    tc = 1
    while tc * 2 <= c4 and tc * 2 <= 32:
        tc *= 2
    tp = 256 // tc
    cgroups = (c4 + tc - 1) // tc
    target = max(1024 // (N * cgroups), 1)
    target = min(target, max((HW + tp * 2 - 1) // (tp * 2), 1))
    chunk = (HW + target - 1) // target
    return {"TC": tc, "TP": tp, "cgroups": cgroups, "chunk": chunk, "nchunk": (HW + chunk - 1) // chunk}


def plan_edges(N, HW, C):
    """Which ragged parts of the plan an (N, HW, C) reduction runs."""
    p = norm_plan(N, HW, C)
    return {"short_last_chunk": HW % p["chunk"] != 0, "partial_channel_group": (C // 4) % p["TC"] != 0,
            "single_chunk": p["nchunk"] == 1, "hw_below_tp": HW < p["TP"], "hw_one": HW == 1, "one_image": N == 1}


def _layer_case(B, layer, act):
    name, cin, cout, k, stride, pad, ups, cphys, h = layer
    ho = (h // ups + 2 * pad - k) // stride + 1
    if act == RELU:
        combo = (RELU, NONE)                             # D / U / R.conv1: conv -> ReLU -> IN
    elif name.startswith("encoder stem"):
        combo = (NONE, RELU)                             # CaSb: conv -> IN -> ReLU
    elif name.startswith("discriminator"):
        combo = (NONE, LEAKY)
    else:
        combo = (NONE, NONE)                             # R.conv2: conv -> IN, + the block's input
    shuffle = name.startswith(("U1", "U2", "U3"))        # U blocks store through the next block's PixelShuffle
    residual = name.startswith("R ") and act == NONE
    return (f"B{B} {name} act{act}", (B, ho, ho, cout), combo, shuffle, residual)


MODEL_CASES = [_layer_case(B, l, a) for B, l, a in NORM_CASES]
# each one chosen for a condition of the plan (test_native_abi.py checks that they still hit them)
RAGGED_CASES = [
    (3, 17, 13, 20),       # short last chunk + partial channel group
    (2, 9, 7, 12),         # partial channel group, HW < TP
    (2, 5, 11, 36),        # partial channel group, one chunk
    (1, 2, 2, 1024),       # HW < TP, one image
    (4, 1, 1, 64),         # HW == 1
    (3, 17, 13, 48),       # short last chunk + partial group, shuffle-able
    (3, 17, 13, 96),       # ditto, 7 chunks
    (2, 45, 37, 132),      # 105 chunks, the last one pixel long; a group with a single quad
    (1, 33, 31, 64),       # one image, 32 chunks, short last
]
IN_SHAPES = [c[1] for c in MODEL_CASES] + RAGGED_CASES


# ------------------------------------------------------------------ helpers
def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Out:
    """An output buffer prefilled with `fill`, followed by GUARD sentinel words."""

    def __init__(self, shape, device, fill=NAN):
        self.n = math.prod(shape)
        self.buf = torch.empty(self.n + GUARD, dtype=torch.float32, device=device)
        self.buf[self.n:].view(torch.int32).fill_(SENTINEL)
        self.t = self.buf[:self.n].view(shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill)
        else:
            self.t.fill_(fill)

    def check(self, what):
        assert (self.buf[self.n:].view(torch.int32) == SENTINEL).all().item(), f"{what}: the kernel wrote past the end of its output"
        return self.t


def _call(pkg, name, *args):
    lib = pkg._native.lib()
    pkg._native.check(getattr(lib, name)(*args), name)


def _ws(nbytes, device):
    return torch.full((max(int(nbytes), 16) // 4 + 4,), NAN, dtype=torch.float32, device=device)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


REPORT = {}        # entry point -> largest error seen, as a multiple of its tolerance (VCG_ERROR_REPORT=<file> writes it out)


def _note(key, value):
    REPORT[key] = max(REPORT.get(key, 0.0), float(value))
    return value


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    if os.environ.get("VCG_ERROR_REPORT"):
        with open(os.environ["VCG_ERROR_REPORT"], "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _worst(err, tol, key=None):
    """max of err / tol (NaN counts as a miss)"""
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    w = r.max().item() if r.numel() else 0.0
    return _note(key, w) if key else w


def _randn(shape, device, seed, dtype=torch.float32):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(shape, generator=g, device=device, dtype=dtype)


def _rand(shape, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.rand(shape, generator=g, device=device)


# ------------------------------------------------------------------ 1. InstanceNorm
def _in_input(shape, device, seed, epi, special=True):
    """NHWC activation with per-(image, channel) offsets and spreads; channel 1 has a mean 10^3 x its spread, the last channel is
    a dead (all-zero) plane, channel 2 of image 0 a constant 0.37 plane."""
    N, H, W, C = shape
    z = _randn(shape, device, seed)
    spread = torch.exp(_randn((N, 1, 1, C), device, seed + 1) * 0.5)
    off = _randn((N, 1, 1, C), device, seed + 2) * spread
    if special:
        off[..., 1] = 1000.0 * spread[..., 1]
    t = z * spread + off
    if epi == RELU:
        t = torch.relu(t)
    if special:
        t[..., C - 1] = 0.0
        if C > 8:
            t[0, :, :, 2] = 0.37
    return t.contiguous()


def _stats_ref(t):
    tn = nchw(t).double()
    m = tn.mean((2, 3))
    v = tn.var((2, 3), unbiased=False)
    return m, v, 1.0 / torch.sqrt(v + EPS)


def _run_stats(pkg, t, device):
    N, H, W, C = t.shape
    lib = pkg._native.lib()
    mean, rstd = Out((N, C), device), Out((N, C), device)
    ws = _ws(lib.vcg_in_workspace(N, H * W, C), device)
    _call(pkg, "vcg_in_stats", P(t), P(mean.t), P(rstd.t), N, H * W, C, EPS, P(ws), ws.numel() * 4, _st())
    return mean, rstd


def _check_stats(pkg, t, device):
    N, H, W, C = t.shape
    mean, rstd = _run_stats(pkg, t, device)
    torch.cuda.synchronize()
    m, r = mean.check("vcg_in_stats mean"), rstd.check("vcg_in_stats rstd")
    m64, v64, r64 = _stats_ref(t)
    tn = nchw(t).double()
    HW = H * W
    # mean: a double sum rounded once; rstd: 1 / sqrt(var + eps) of double sums, rounded once
    tol_m = U * m64.abs() + 2.0 ** -53 * HW * tn.abs().mean((2, 3)) + 1e-300
    tol_r = (U + 0.5 * 2.0 ** -53 * (HW + 4) * 2 * (tn * tn).mean((2, 3)) / (v64 + EPS)) * r64
    wm, wr = _worst((m.double() - m64).abs(), tol_m, "in_stats mean"), _worst((r.double() - r64).abs(), tol_r, "in_stats rstd")
    assert wm <= 1, f"vcg_in_stats: mean off by {wm:.2f} x its fp32 rounding bound"
    assert wr <= 1, f"vcg_in_stats: rstd off by {wr:.2f} x its fp32 rounding bound"
    const = v64 == 0
    assert ((r.double() - r64).abs()[const] <= U * r64[const]).all(), "constant planes: rstd is not 1 / sqrt(eps)"
    # bitwise reproducible
    mean2, rstd2 = _run_stats(pkg, t, device)
    torch.cuda.synchronize()
    assert torch.equal(mean2.t, m) and torch.equal(rstd2.t, r), "vcg_in_stats: two runs on the same input differ"
    return m, r


def _act64(x, act):
    if act == RELU:
        return torch.relu(x)
    if act == LEAKY:
        return F.leaky_relu(x, 0.2)
    if act == TANH:
        return torch.tanh(x)
    if act == SIGMOID:
        return torch.sigmoid(x)
    return x


def _act_kinked(y, act, side):
    """post_act of the float64 normalised value, with the ReLU / LeakyReLU kink on `side` (bool, the fp32 value > 0)"""
    if act == RELU:
        return torch.where(side, y, torch.zeros_like(y))
    if act == LEAKY:
        return torch.where(side, y, 0.2 * y)
    return _act64(y, act)


def _act_grad_in(x, act, side):
    if act == RELU:
        return side.to(x.dtype)
    if act == LEAKY:
        return torch.where(side, torch.ones_like(x), torch.full_like(x, 0.2))
    if act == TANH:
        return 1 - torch.tanh(x) ** 2
    if act == SIGMOID:
        s = torch.sigmoid(x)
        return s * (1 - s)
    return torch.ones_like(x)


def _epi_grad(t, epi):
    """epi'(t) from the activation OUTPUT t (torch's threshold_backward / leaky_relu_backward conventions)"""
    if epi == RELU:
        return (t > 0).to(t.dtype)
    if epi == LEAKY:
        return torch.where(t > 0, torch.ones_like(t), torch.full_like(t, 0.2))
    return torch.ones_like(t)


def _apply(pkg, t, mean, rstd, residual, post, shuffle, device):
    N, H, W, C = t.shape
    shape = (N, 2 * H, 2 * W, C // 4) if shuffle else (N, H, W, C)
    out = Out(shape, device)
    h = ctypes.c_uint64(0)
    _call(pkg, "vcg_in_apply_h", P(t), P(mean), P(rstd), P(residual), P(out.t), N, H, W, C, post, int(shuffle), ctypes.byref(h), _st())
    return out, h.value


def _check_apply(pkg, t, m, r, post, shuffle, residual, device):
    out, h = _apply(pkg, t, m, r, residual, post, shuffle, device)
    torch.cuda.synchronize()
    got = out.check(f"vcg_in_apply post={ACTS[post]} shuffle={shuffle}").double()
    assert h != 0 and (h >> 56) == 0xA5
    m64, _, r64 = _stats_ref(t)
    xh = (nchw(t).double() - m64[:, :, None, None]) * r64[:, :, None, None]
    ref = _act64(xh, post)
    # xhat's error through the fp32 mean and rstd, the activation's own rounding, and the rounding of the sum with the residual
    tol = 8 * U * (xh.abs() + (r64 * m64.abs())[:, :, None, None] + ref.abs())
    if residual is not None:
        ref = ref + nchw(residual).double()
        tol = tol + U * ref.abs()
    if shuffle:
        ref, tol = F.pixel_shuffle(ref, 2), F.pixel_shuffle(tol, 2)
    w = _worst((nchw(got) - ref).abs(), tol, "in_apply_h")
    assert w <= 1, f"vcg_in_apply post={ACTS[post]} shuffle={shuffle} residual={residual is not None}: {w:.2f} x the rounding bound"
    return w


def _bwd(pkg, g, t, m, r, epi, post, shuffle, device, gbias=None, c_log=0):
    N, H, W, C = t.shape
    lib = pkg._native.lib()
    dt = Out((N, H, W, C), device)
    ws = _ws(lib.vcg_in_workspace(N, H * W, C), device)
    h = ctypes.c_uint64(0)
    if gbias is None:
        _call(pkg, "vcg_in_bwd_h", P(g), P(t), P(m), P(r), P(dt.t), N, H, W, C, epi, post, int(shuffle), P(ws), ws.numel() * 4,
              ctypes.byref(h), _st())
    else:
        _call(pkg, "vcg_in_bwd_bias", P(g), P(t), P(m), P(r), P(dt.t), N, H, W, C, epi, post, int(shuffle), P(gbias), c_log, P(ws),
              ws.numel() * 4, ctypes.byref(h), _st())
    return dt, h.value


def _in64(x):
    """F.instance_norm (no affine, biased variance) written out, so that it also takes 1 x 1 planes"""
    m = x.mean((2, 3), keepdim=True)
    v = x.var((2, 3), unbiased=False, keepdim=True)
    return (x - m) / torch.sqrt(v + EPS)


def _bwd_refs(t, m32, r32, g, epi, post, shuffle):
    """(float64 autograd dt, torch fp32 autograd dt, elementwise rounding bound) in NCHW"""
    tn = nchw(t)
    side = ((tn - m32[:, :, None, None]) * r32[:, :, None, None]) > 0        # the fp32 normalised value's side of a kink
    gn = nchw(g)
    x = tn.double().requires_grad_(True)
    y = _act_kinked(_in64(x), post, side)
    if shuffle:
        y = F.pixel_shuffle(y, 2)
    y.backward(gn.double())
    epi64 = _epi_grad(tn.double(), epi)
    ref = x.grad * epi64
    tref = None
    if tn.shape[2] * tn.shape[3] > 1:
        x32 = tn.clone().requires_grad_(True)
        y32 = _act64(F.instance_norm(x32, eps=EPS), post)
        if shuffle:
            y32 = F.pixel_shuffle(y32, 2)
        y32.backward(gn)
        tref = x32.grad.double() * epi64
    # the rounding bound, per plane: X = max |xhat| + rstd |mean| + 1 bounds xhat's error (in units of U) through the fp32 mean and
    # rstd; it reaches dt directly (times s2, and g'' for Tanh / Sigmoid) and through s1 = mean(g') and s2 = mean(g' xhat)
    m64, _, r64 = _stats_ref(t)
    xh = (tn.double() - m64[:, :, None, None]) * r64[:, :, None, None]
    gu = F.pixel_unshuffle(gn.double(), 2) if shuffle else gn.double()
    gp = gu * _act_grad_in(xh, post, side)
    s1, s2 = gp.mean((2, 3)), (gp * xh).mean((2, 3))
    xm = xh.abs().amax((2, 3))
    X = xm + r64 * m64.abs() + 1
    curv = X if post in (TANH, SIGMOID) else 0
    scale = r64 * (gu.abs().amax((2, 3)) * (1 + curv + xm * xm) + s1.abs() * (1 + xm * X) + s2.abs() * X * (1 + xm))
    return ref, tref, 16 * U * scale[:, :, None, None].expand_as(ref), r64


def _check_bwd(pkg, t, m, r, g, epi, post, shuffle, device, vs_torch=False, what=""):
    dt, h = _bwd(pkg, g, t, m, r, epi, post, shuffle, device)
    torch.cuda.synchronize()
    got = nchw(dt.check(f"vcg_in_bwd {what}")).double()
    assert h != 0 and (h >> 56) == 0xA5
    ref, tref, tol, _ = _bwd_refs(t, m, r, g, epi, post, shuffle)
    w = _worst((got - ref).abs(), tol, "in_bwd_h")
    assert w <= 1, f"vcg_in_bwd {what} epi={ACTS[epi]} post={ACTS[post]} shuffle={shuffle}: {w:.2f} x the rounding bound"
    if vs_torch:
        ek, et = (got - ref).norm().item(), (tref - ref).norm().item()
        _note("in_bwd_h / torch fp32 (L2)", ek / max(et, 1e-300))
        assert ek <= 4 * et + U * ref.norm().item(), f"vcg_in_bwd {what}: error {ek:.3e} vs PyTorch fp32's {et:.3e}"
    # bitwise reproducible
    dt2, _ = _bwd(pkg, g, t, m, r, epi, post, shuffle, device)
    torch.cuda.synchronize()
    assert torch.equal(dt2.t, dt.t), f"vcg_in_bwd {what}: two runs on the same inputs differ"
    return dt.t, w


def _check_bwd_bias(pkg, t, m, r, g, epi, post, shuffle, dt_plain, c_log, device):
    N, H, W, C = t.shape
    pre = _randn((C,), device, 99) * 3.0
    gb = Out((C,), device, fill=pre)
    dt, h = _bwd(pkg, g, t, m, r, epi, post, shuffle, device, gbias=gb.t, c_log=c_log)
    gb2 = Out((C,), device, fill=pre)
    _bwd(pkg, g, t, m, r, epi, post, shuffle, device, gbias=gb2.t, c_log=c_log)
    torch.cuda.synchronize()
    got = gb.check("vcg_in_bwd_bias gbias").double()
    assert h != 0 and (h >> 56) == 0xA5
    assert torch.equal(dt.check("vcg_in_bwd_bias dt"), dt_plain), "vcg_in_bwd_bias: dt differs from vcg_in_bwd_h's"
    assert torch.equal(gb2.t, gb.t), "vcg_in_bwd_bias: two runs on the same inputs differ"
    d = dt_plain.double().reshape(-1, C)
    cs = d.sum(0)
    p = norm_plan(N, H * W, C)
    # fp32 tree: chunk/TP per lane, TP lanes, N nchunk / 128 per row lane x 4, 32 row lanes, + the add into the prefill
    L = -(-p["chunk"] // p["TP"]) + p["TP"] + -(-N * p["nchunk"] // 128) + 36
    tol = U * (L * d.abs().sum(0) + (pre.double() + cs).abs()) + 1e-300
    w = _worst((got[:c_log] - pre.double()[:c_log] - cs[:c_log]).abs(), tol[:c_log], "in_bwd_bias gbias")
    assert w <= 1, f"vcg_in_bwd_bias: column sums off by {w:.2f} x the fp32 summation bound"
    assert torch.equal(gb.t[c_log:], pre[c_log:]), "vcg_in_bwd_bias: gbias[c_log:] was written"
    return w


@pytest.mark.parametrize("case", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_instance_norm_at_model_size(case, pkg, device):
    """Stats, apply, backward and bias gradient of every normalised layer of BASELINE configs[1-3] at full size, with the
    (epilogue, post-activation, shuffle, residual) the model runs it with."""
    name, shape, (epi, post), shuffle, residual = case
    seed = zlib.crc32(name.encode()) % (1 << 30)
    t = _in_input(shape, device, seed, epi)
    m, r = _check_stats(pkg, t, device)
    res = (_randn(shape, device, seed + 3)) if residual else None
    _check_apply(pkg, t, m, r, post, shuffle, res, device)
    N, H, W, C = shape
    gshape = (N, 2 * H, 2 * W, C // 4) if shuffle else shape
    g = _randn(gshape, device, seed + 4)
    dt, _ = _check_bwd(pkg, t, m, r, g, epi, post, shuffle, device, vs_torch=True, what=name)
    if epi == RELU:
        _check_bwd_bias(pkg, t, m, r, g, epi, post, shuffle, dt, C, device)


BWD_COMBOS = [(RELU, NONE), (NONE, RELU), (NONE, LEAKY), (NONE, NONE), (NONE, TANH), (NONE, SIGMOID)]


@pytest.mark.parametrize("shape", RAGGED_CASES, ids=["x".join(map(str, c)) for c in RAGGED_CASES])
def test_instance_norm_ragged_plans(shape, pkg, device):
    """The short last chunk, partial channel groups, HW < TP, HW == 1 and one-image plans: every post-activation with and without a
    residual and through the shuffle, every backward combination, the bias gradient with c_log < C."""
    N, H, W, C = shape
    seed = N * 1000003 + H * 1009 + W * 17 + C
    for epi in (NONE, RELU):
        t = _in_input(shape, device, seed + epi, epi)
        m, r = _check_stats(pkg, t, device)
        if epi == NONE:
            res = _randn(shape, device, seed + 7)
            for post in ACTS:
                _check_apply(pkg, t, m, r, post, False, None, device)
                _check_apply(pkg, t, m, r, post, False, res, device)
                if C % 16 == 0:
                    _check_apply(pkg, t, m, r, post, True, None, device)
        g = _randn(shape, device, seed + 11)
        for e, post in BWD_COMBOS:
            if e != epi:
                continue
            dt, _ = _check_bwd(pkg, t, m, r, g, epi, post, False, device, what=f"{shape}")
            if epi == RELU:
                _check_bwd_bias(pkg, t, m, r, g, epi, post, False, dt, C - 3 if C > 4 else C, device)
        if C % 16 == 0:
            gs = _randn((N, 2 * H, 2 * W, C // 4), device, seed + 13)
            dt, _ = _check_bwd(pkg, t, m, r, gs, epi, NONE, True, device, what=f"{shape} shuffled")
            if epi == RELU:
                _check_bwd_bias(pkg, t, m, r, gs, epi, NONE, True, dt, C, device)


@pytest.mark.parametrize("shape,epi", [((8, 16, 16, 1024), NONE), ((8, 128, 128, 128), RELU), ((3, 17, 13, 20), NONE)],
                         ids=["R.conv2 B8", "D1 B8", "ragged"])
def test_instance_norm_backward_cancellation(shape, epi, pkg, device):
    """g = a xhat + b + 1e-3 noise: g' - s1 - xhat s2 keeps 1e-3 of its terms.  The error, measured against rstd ||g||, must stay
    at fp32 rounding and no worse than 4x PyTorch's fp32 backward."""
    N, H, W, C = shape
    t = _in_input(shape, device, 4242 + C, epi, special=False)
    m, r = _check_stats(pkg, t, device)
    m64, _, r64 = _stats_ref(t)
    xh = ((nchw(t).double() - m64[:, :, None, None]) * r64[:, :, None, None])
    a = _randn((N, C, 1, 1), device, 5, torch.float64) * 2
    b = _randn((N, C, 1, 1), device, 6, torch.float64) * 2
    gn = a * xh + b + 1e-3 * _randn((N, C, H, W), device, 7, torch.float64)
    g = nhwc(gn).float().contiguous()
    dt, _ = _bwd(pkg, g, t, m, r, epi, NONE, False, device)
    torch.cuda.synchronize()
    got = nchw(dt.check("vcg_in_bwd")).double()
    ref, tref, tol, _ = _bwd_refs(t, m, r, g, epi, NONE, False)
    assert _worst((got - ref).abs(), tol, "in_bwd_h") <= 1
    rg = (r64[:, :, None, None] * nchw(g).double()).norm().item()
    ek, et = (got - ref).norm().item(), (tref - ref).norm().item()
    _note("in_bwd_h cancelling: error / (U rstd |g|)", ek / (U * rg))
    _note("in_bwd_h cancelling / torch fp32 (L2)", ek / et)
    assert ek <= 16 * U * rg, f"cancelling backward: error {ek / rg:.3e} of rstd ||g||"
    assert ek <= 4 * et + U * rg, f"cancelling backward: error {ek:.3e} vs PyTorch fp32's {et:.3e}"


# ------------------------------------------------------------------ 2. activation backward and layout helpers
def _act_out(z, act):
    return _act64(z, act).float() if act != NONE else z


@pytest.mark.parametrize("act", list(ACTS), ids=list(ACTS.values()))
def test_act_bwd_all_activations(act, pkg, device):
    n = 2048 * 256 * 4 + 4 * 1234                    # the 2048-block grid-stride loop wraps
    t = _act_out(_randn((n,), device, 30 + act) * 2, act).contiguous()
    t[0], t[1], t[n - 1], t[n - 2] = 0.0, -0.0, 0.0, -0.0
    g = _randn((n,), device, 40 + act)
    dt = Out((n,), device)
    h = ctypes.c_uint64(0)
    _call(pkg, "vcg_act_bwd_h", P(g), P(t), P(dt.t), n, act, ctypes.byref(h), _st())
    torch.cuda.synchronize()
    got = dt.check("vcg_act_bwd").double()
    td, gd = t.double(), g.double()
    if act == RELU:
        d = (td > 0).double()
    elif act == LEAKY:
        d = torch.where(td > 0, torch.ones_like(td), torch.full_like(td, 0.2))
    elif act == TANH:
        d = 1 - td * td
    elif act == SIGMOID:
        d = td * (1 - td)
    else:
        d = torch.ones_like(td)
    ref = gd * d
    tol = 4 * U * gd.abs() * (d.abs() + td * td + td.abs())
    assert _worst((got - ref).abs(), tol + 1e-300, "act_bwd_h") <= 1, f"vcg_act_bwd {ACTS[act]}"
    z = [0, 1, n - 1, n - 2]
    if act == RELU:
        assert (got[z] == 0).all(), "t = +-0 must take the t <= 0 branch"
    if act == LEAKY:
        assert torch.equal(dt.t[z], g[z] * 0.2), "t = +-0 must take the t <= 0 branch"
    assert h != 0


@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (3, 17, 13, 96), (8, 32, 32, 512)])
def test_pixel_shuffle_forward_and_inverse(shape, pkg, device):
    N, H, W, C = shape
    x = _randn(shape, device, 50 + C)
    out = Out((N, 2 * H, 2 * W, C // 4), device)
    _call(pkg, "vcg_pixel_shuffle", P(x), P(out.t), N, H, W, C, 0, _st())
    back = Out(shape, device)
    big = _randn((N, 2 * H, 2 * W, C // 4), device, 51 + C)
    _call(pkg, "vcg_pixel_shuffle", P(big), P(back.t), N, H, W, C, 1, _st())
    torch.cuda.synchronize()
    assert torch.equal(out.check("vcg_pixel_shuffle"), nhwc(F.pixel_shuffle(nchw(x), 2)))
    assert torch.equal(back.check("vcg_pixel_shuffle inverse"), nhwc(F.pixel_unshuffle(nchw(big), 2)))


@pytest.mark.parametrize("rows,ca,cb", [(1, 4, 4), (1000, 64, 64), (777, 12, 1024)])
def test_chan_split_cat_and_add_into(rows, ca, cb, pkg, device):
    src = _randn((rows, ca + cb), device, 60 + ca)
    a, b = Out((rows, ca), device), Out((rows, cb), device)
    _call(pkg, "vcg_chan_split", P(src), P(a.t), P(b.t), rows, ca, cb, _st())
    cat = Out((rows, ca + cb), device)
    xa, xb = _randn((rows, ca), device, 61), _randn((rows, cb), device, 62)
    _call(pkg, "vcg_chan_cat", P(xa), P(xb), P(cat.t), rows, ca, cb, _st())
    cat_a, cat_b = Out((rows, ca + cb), device), Out((rows, ca + cb), device)
    _call(pkg, "vcg_chan_cat", None, P(xb), P(cat_a.t), rows, ca, cb, _st())
    _call(pkg, "vcg_chan_cat", P(xa), None, P(cat_b.t), rows, ca, cb, _st())
    torch.cuda.synchronize()
    assert torch.equal(a.check("vcg_chan_split a"), src[:, :ca]) and torch.equal(b.check("vcg_chan_split b"), src[:, ca:])
    assert torch.equal(cat.check("vcg_chan_cat"), torch.cat([xa, xb], 1))
    assert torch.equal(cat_a.check("vcg_chan_cat"), torch.cat([torch.zeros_like(xa), xb], 1))
    assert torch.equal(cat_b.check("vcg_chan_cat"), torch.cat([xa, torch.zeros_like(xb)], 1))
    n = rows * (ca + cb)
    dst = Out((n,), device, fill=_randn((n,), device, 63))
    sadd = Out((n,), device, fill=_randn((n,), device, 64))
    want = dst.t + sadd.t
    _call(pkg, "vcg_add_into", P(dst.t), P(sadd.t), n, _st())
    torch.cuda.synchronize()
    assert torch.equal(dst.check("vcg_add_into dst"), want)
    assert (sadd.check("vcg_add_into src").view(torch.int32) == 0).all(), "vcg_add_into: src is not +0 afterwards"


# ------------------------------------------------------------------ 3. amax handles
E = 6
BIG = -1.9999 * 2.0 ** E                       # every other element stays below 2^(E-2)


def _consumer_fwd(pkg, x, device, handle):
    """y = conv1x1(x) on the split-operand forward, x's scale taken from `handle` (0: measured)"""
    N, H, W, C = x.shape
    spec = pkg.ops.ConvSpec(C, 64, 1, 1, 0, False, 1)
    w = _randn((64, C, 1, 1), device, 70 + C) * 0.1
    cd = spec.desc(N, H, W)
    ws = _ws(pkg._native.lib().vcg_conv_fwd_workspace(cd), device)
    y = torch.full((N, H, W, 64), NAN, device=device)
    bias = torch.zeros(64, device=device)
    _call(pkg, "vcg_conv_fwd_in_h", P(x), P(spec.packed(w)), P(bias), P(y), None, None, EPS, None, cd, P(ws), ws.numel() * 4, handle, _st())
    torch.cuda.synchronize()
    return y


def _consumer_dgrad(pkg, dy, device, handle):
    """dx = conv1x1^T(dy), zero padding (the operand bound is amax(dy) itself), dy's scale from `handle`"""
    N, H, W, C = dy.shape
    spec = pkg.ops.ConvSpec(64, C, 1, 1, 0, False, 1)
    w = _randn((C, 64, 1, 1), device, 71 + C) * 0.1
    cd = spec.desc(N, H, W)
    ws = _ws(pkg._native.lib().vcg_conv_dgrad_workspace(cd), device)
    dx = torch.full((N, H, W, 64), NAN, device=device)
    _call(pkg, "vcg_conv_dgrad_h", P(dy), P(spec.packed(w)), P(dx), cd, P(ws), ws.numel() * 4, handle, _st())
    torch.cuda.synchronize()
    return dx


def _handle_ok(pkg, consumer, tensor, handle, device, what):
    assert handle != 0 and pkg._native.lib().vcg_amax_valid(handle), f"{what}: no valid handle"
    assert tensor.abs().max().item() >= 2.0 ** E and (tensor.abs() >= 2.0 ** (E - 2)).sum().item() == 1, f"{what}: the plant is not unique"
    a, b = consumer(pkg, tensor, device, handle), consumer(pkg, tensor, device, 0)
    assert torch.isfinite(b).all()
    assert torch.isfinite(a).all() and torch.equal(a, b), f"{what}: the published amax under-reports the tensor it describes"


AMAX_SHAPE = (3, 17, 13, 96)
# (image, pixel, channel): the first element, the last pixel of the last image in the last channel group, inside the short last chunk
AMAX_SPOTS = [(0, 0, 0), (2, 17 * 13 - 1, 95), (1, 200, 50)]


def test_amax_consumers_trust_the_handle(pkg, device):
    """Positive control of the tests below: a handle that under-reports by three binades makes both consumers overflow."""
    lib = pkg._native.lib()
    x = _randn(AMAX_SHAPE, device, 80) * 0.5
    x.view(-1)[5] = BIG
    decoy = torch.full((64,), 1.5 * 2.0 ** (E - 3), device=device)
    h = lib.vcg_amax_measure(P(decoy), 64, _st())
    assert h != 0
    for consumer in (_consumer_fwd, _consumer_dgrad):
        assert torch.isfinite(consumer(pkg, x, device, 0)).all()
        assert not torch.isfinite(consumer(pkg, x, device, h)).all(), f"{consumer.__name__} does not take the handle"


@pytest.mark.parametrize("mode", ["plain", "residual", "shuffle", "wrap"])
def test_amax_of_in_apply(mode, pkg, device):
    N, H, W, C = (2, 64, 66, 256) if mode == "wrap" else AMAX_SHAPE
    HW = H * W
    mean = torch.zeros((N, C), device=device)
    rstd = torch.ones((N, C), device=device)
    spots = [(N - 1, HW - 1, C - 1)] if mode == "wrap" else AMAX_SPOTS
    if mode == "shuffle":
        spots = [(1, 100, 4 * 7 + e) for e in range(4)]          # the four sub-positions of one quad
    for n, pix, c in spots:
        t = _randn((N, H, W, C), device, 81) * 0.5
        res = _randn((N, H, W, C), device, 82) * 0.5 if mode == "residual" else None
        (res if res is not None else t)[n, pix // W, pix % W, c] = BIG
        out, h = _apply(pkg, t, mean, rstd, res, NONE, mode == "shuffle", device)
        torch.cuda.synchronize()
        o = out.check("vcg_in_apply")
        _handle_ok(pkg, _consumer_fwd, o, h, device, f"vcg_in_apply {mode} at {(n, pix, c)}")


@pytest.mark.parametrize("mode", ["plain", "bias", "shuffle"])
def test_amax_of_in_bwd(mode, pkg, device):
    N, H, W, C = AMAX_SHAPE
    mean = torch.zeros((N, C), device=device)
    rstd = torch.ones((N, C), device=device)
    t = _randn(AMAX_SHAPE, device, 83) * 0.5
    if mode == "shuffle":
        spots = [(1, 2 * 7 + i, 2 * 5 + j, 9) for i in (0, 1) for j in (0, 1)]          # g at the four shuffled sub-positions
        gshape = (N, 2 * H, 2 * W, C // 4)
    else:
        spots = [(n, pix // W, pix % W, c) for n, pix, c in AMAX_SPOTS]
        gshape = AMAX_SHAPE
    for spot in spots:
        g = _randn(gshape, device, 84) * 0.5
        g[spot] = BIG
        gb = torch.zeros((C,), device=device) if mode == "bias" else None
        dt, h = _bwd(pkg, g, t, mean, rstd, NONE, NONE, mode == "shuffle", device, gbias=gb, c_log=C)
        torch.cuda.synchronize()
        _handle_ok(pkg, _consumer_dgrad, dt.check("vcg_in_bwd"), h, device, f"vcg_in_bwd {mode} at {spot}")


def test_amax_of_act_bwd(pkg, device):
    shape = (2, 110, 110, 96)                      # 580800 quads: the 2048 x 256 grid-stride loop wraps
    n = math.prod(shape)
    t = _randn((n,), device, 85)
    for i in (0, n - 1, 2048 * 256 * 4 + 9):
        g = _randn((n,), device, 86) * 0.5
        g[i] = BIG
        dt = Out((n,), device)
        h = ctypes.c_uint64(0)
        _call(pkg, "vcg_act_bwd_h", P(g), P(t), P(dt.t), n, NONE, ctypes.byref(h), _st())
        torch.cuda.synchronize()
        _handle_ok(pkg, _consumer_dgrad, dt.check("vcg_act_bwd").view(shape), h.value, device, f"vcg_act_bwd at {i}")


# ------------------------------------------------------------------ 4. reparameterisation and losses
def _edge_lv(n, device, seed):
    lv = _randn((n,), device, seed) * 8
    ten = torch.tensor(10.0, dtype=torch.float32)
    edges = [10.0, -10.0, torch.nextafter(ten, torch.tensor(0.0)).item(), torch.nextafter(ten, torch.tensor(99.0)).item(),
             -torch.nextafter(ten, torch.tensor(0.0)).item(), -torch.nextafter(ten, torch.tensor(99.0)).item(), 12.0, -12.0, 60.0, -60.0]
    lv[:len(edges)] = torch.tensor(edges, device=device)
    lv[n - len(edges):] = torch.tensor(edges, device=device)
    return lv


def test_reparam_fwd_given_eps(pkg, device):
    n = 4099
    mu, eps = _randn((n,), device, 90), _randn((n,), device, 91)
    lv = _edge_lv(n, device, 92)
    z, lvc = Out((n,), device), Out((n,), device)
    _call(pkg, "vcg_reparam_fwd", P(mu), P(lv), P(eps), None, P(z.t), P(lvc.t), n, 0, 0, _st())
    torch.cuda.synchronize()
    assert torch.equal(lvc.check("vcg_reparam_fwd lvc"), lv.clamp(-10, 10))
    l64 = lv.double().clamp(-10, 10)
    sd = torch.exp(0.5 * l64)
    ref = mu.double() + eps.double() * sd
    tol = 4 * U * (mu.double().abs() + 2 * (eps.double() * sd).abs())
    assert _worst((z.check("vcg_reparam_fwd z").double() - ref).abs(), tol + 1e-300, "reparam_fwd z") <= 1


def test_reparam_fwd_draws_eps_like_randn(pkg, device):
    n = 4 * 777 + 3
    mu, lv = _randn((n,), device, 93), _edge_lv(n, device, 94)
    z, lvc, eo = Out((n,), device), Out((n,), device), Out((n,), device)
    _call(pkg, "vcg_reparam_fwd", P(mu), P(lv), None, P(eo.t), P(z.t), P(lvc.t), n, 1234, 5678, _st())
    rn = Out((n,), device)
    _call(pkg, "vcg_randn", P(rn.t), n, 1234, 5678, _st())
    torch.cuda.synchronize()
    assert torch.equal(eo.check("vcg_reparam_fwd eps_out"), rn.check("vcg_randn"))
    ref = mu.double() + eo.t.double() * torch.exp(0.5 * lv.double().clamp(-10, 10))
    tol = 4 * U * (mu.double().abs() + 2 * (ref - mu.double()).abs())
    assert _worst((z.check("z").double() - ref).abs(), tol + 1e-300, "reparam_fwd z") <= 1


@pytest.mark.parametrize("which", ["both", "no_gz", "no_glvc"])
def test_reparam_bwd_closed_interval(which, pkg, device):
    n = 4099
    lv = _edge_lv(n, device, 95)
    eps, gz, glvc = _randn((n,), device, 96), _randn((n,), device, 97), _randn((n,), device, 98)
    gz_ = None if which == "no_gz" else gz
    gl_ = None if which == "no_glvc" else glvc
    dmu, dlv = Out((n,), device), Out((n,), device)
    _call(pkg, "vcg_reparam_bwd", P(gz_), P(gl_), P(eps), P(lv), P(dmu.t), P(dlv.t), n, _st())
    torch.cuda.synchronize()
    mu64 = torch.zeros(n, dtype=torch.float64, device=device, requires_grad=True)
    lv64 = lv.double().requires_grad_(True)
    lvc = torch.clamp(lv64, -10, 10)
    z = mu64 + eps.double() * torch.exp(0.5 * lvc)
    loss = 0
    if gz_ is not None:
        loss = loss + (z * gz.double()).sum()
    if gl_ is not None:
        loss = loss + (lvc * glvc.double()).sum()
    loss.backward()
    assert torch.equal(dmu.check("vcg_reparam_bwd dmu"), gz if gz_ is not None else torch.zeros_like(gz))
    a = (gz.double() * eps.double() * 0.5 * torch.exp(0.5 * lv.double().clamp(-10, 10))).abs() if gz_ is not None else 0
    tol = 6 * U * (a + (glvc.double().abs() if gl_ is not None else 0))
    got = dlv.check("vcg_reparam_bwd dlv").double()
    assert _worst((got - lv64.grad).abs(), tol + 1e-300, "reparam_bwd dlv") <= 1
    inside = (lv >= -10) & (lv <= 10)
    assert (got[~inside] == 0).all() and (got[lv.abs() == 10] != 0).all(), "the clamp gradient is not the closed interval"


def _red_depth(n):
    nb = max(min((n // 4 + 255) // 256, 1024), 1)
    return 4 * -(-(n // 4) // (nb * 256)) + 4 + -(-(n % 4) // 256) + 6 + 4 + 2


@pytest.mark.parametrize("case", [("pitch4", (2, 37, 29)), ("tail", 1031), ("tiny", 3), ("wrap", 1300001)])
def test_l1_loss(case, pkg, device):
    name, spec = case
    if name == "pitch4":
        a = _rand((*spec, 4), device, 102)
        b = _rand((*spec, 4), device, 103)
        a[..., 3] = 0
        b[..., 3] = 0
        a, b = a.reshape(-1), b.reshape(-1)
        n_log = math.prod(spec) * 3
    else:
        a, b = _rand((spec,), device, 104), _rand((spec,), device, 105)
        n_log = spec
    b[::7] = a[::7]                                # ties
    n = a.numel()
    lib = pkg._native.lib()
    out = Out((1,), device)
    ws = _ws(lib.vcg_reduce_workspace(n), device)
    _call(pkg, "vcg_l1_fwd", P(a), P(b), P(out.t), n, n_log, P(ws), ws.numel() * 4, _st())
    gout = torch.tensor([0.75], device=device)
    ga, gb = Out((n,), device), Out((n,), device)
    _call(pkg, "vcg_l1_bwd", P(a), P(b), P(gout), P(ga.t), P(gb.t), n, n_log, _st())
    torch.cuda.synchronize()
    d = a.double() - b.double()
    ref = d.abs().sum() / n_log
    tol = U * (_red_depth(n) * d.abs().sum() / n_log + ref)
    assert _note("l1_fwd", abs(out.check("vcg_l1_fwd").double().item() - ref.item()) / tol.item()) <= 1
    gref = torch.sign(d) * 0.75 / n_log
    gga = ga.check("vcg_l1_bwd ga").double()
    assert _worst((gga - gref).abs(), 3 * U * gref.abs() + 1e-300, "l1_bwd") <= 1
    assert torch.equal(gb.check("vcg_l1_bwd gb"), -ga.t)
    assert (gga[::7] == 0).all(), "a == b must give a zero gradient"


def test_kl_loss_at_the_clamp_edges(pkg, device):
    n = 64 * 16 * 16 * 8 + 3
    mu, lv = _randn((n,), device, 100), _edge_lv(n, device, 101)
    lib = pkg._native.lib()
    out = Out((1,), device)
    ws = _ws(lib.vcg_reduce_workspace(n), device)
    _call(pkg, "vcg_kl_fwd", P(mu), P(lv), P(out.t), n, P(ws), ws.numel() * 4, _st())
    gout = torch.tensor([1.5], device=device)
    gmu, glv = Out((n,), device), Out((n,), device)
    _call(pkg, "vcg_kl_bwd", P(mu), P(lv), P(gout), P(gmu.t), P(glv.t), n, _st())
    torch.cuda.synchronize()
    mu64, lv64 = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    lc = torch.clamp(lv64, -10, 10)
    terms = 1 + lc - mu64 ** 2 - torch.exp(lc)
    kl = -0.5 * terms.mean()
    (kl * 1.5).backward()
    absum = (1 + lc.abs() + mu64 ** 2 + torch.exp(lc)).detach().sum() * 0.5 / n
    tol = U * ((_red_depth(n) + 6) * absum + abs(kl.item()))
    assert _note("kl_fwd", abs(out.check("vcg_kl_fwd").double().item() - kl.item()) / tol.item()) <= 1
    s = 1.5 / n
    assert _worst((gmu.check("gmu").double() - mu64.grad).abs(), 4 * U * mu64.grad.abs() + 1e-300, "kl_bwd gmu") <= 1
    tol = 4 * U * (lv64.grad.abs() + s * torch.exp(lc.detach()))
    got = glv.check("glv").double()
    assert _worst((got - lv64.grad).abs(), tol, "kl_bwd glv") <= 1
    assert (got[lv.abs() > 10] == 0).all() and (got[lv.abs() == 10] != 0).all()


@pytest.mark.parametrize("n", [1, 5, 64, 65, 200])
def test_mse_const(n, pkg, device):
    d = _randn((n,), device, 110 + n) + 0.3
    c = 0.9
    out = Out((2,), device)
    _call(pkg, "vcg_mse_const_fwd", P(d), c, P(out.t), n, _st())
    gout = torch.tensor([0.6], device=device)
    gd = Out((n,), device)
    _call(pkg, "vcg_mse_const_bwd", P(d), c, P(gout), P(gd.t), n, _st())
    torch.cuda.synchronize()
    o = out.check("vcg_mse_const_fwd").double()
    c32 = torch.tensor(c, dtype=torch.float32).double()
    e = d.double() - c32
    r0, r1 = (e * e).mean().item(), d.double().mean().item()
    assert _note("mse_const_fwd", abs(o[0].item() - r0) / (5 * U * r0)) <= 1
    assert _note("mse_const_fwd mean", abs(o[1].item() - r1) / (U * abs(r1) + 2.0 ** -50 * d.double().abs().mean().item())) <= 1
    gref = e * 0.6 * 2 / n
    assert _worst((gd.check("vcg_mse_const_bwd").double() - gref).abs(), 4 * U * gref.abs() + 1e-300, "mse_const_bwd") <= 1


@pytest.mark.parametrize("count", [1, 16])
def test_lincomb(count, pkg, device):
    vals = _randn((count,), device, 120 + count)
    ws = [0.5 + 0.37 * i for i in range(count)]
    ptrs = (ctypes.c_void_p * count)(*[vals.data_ptr() + 4 * i for i in range(count)])
    wts = (ctypes.c_float * count)(*ws)
    out = Out((1,), device)
    pkg._native.check(pkg._native.lib().vcg_lincomb_fwd(ptrs, wts, count, P(out.t), _st()), "vcg_lincomb_fwd")
    torch.cuda.synchronize()
    w64 = torch.tensor(list(wts), dtype=torch.float64, device=device)
    terms = w64 * vals.double()
    ref = terms.sum().item()
    assert _note("lincomb_fwd", abs(out.check("vcg_lincomb_fwd").double().item() - ref) / ((count + 2) * U * terms.abs().sum().item())) <= 1


# ------------------------------------------------------------------ 5. spectral norm and the full-map discriminator conv
def _sn_depth(K):
    return 4 * -(-(K // 4) // 1024) + 4 + 6 + 16


def _sn_run(pkg, w, u0, v0, C, KH, KW, update, device):
    K = C * KH * KW
    u = torch.tensor([u0], dtype=torch.float32, device=device)
    v = v0.clone()
    sigma, wsn = Out((1,), device), Out((K,), device)
    ws = _ws(64, device)
    _call(pkg, "vcg_sn_prepare", P(w), P(u), P(v), P(sigma.t), P(wsn.t), C, KH, KW, update, P(ws), 64, _st())
    torch.cuda.synchronize()
    return u, v, sigma.check("vcg_sn_prepare sigma"), wsn.check("vcg_sn_prepare wsn_k")


SN_SHAPES = [(512, 16, 16), (64, 4, 4), (20, 3, 5)]


@pytest.mark.parametrize("shape", SN_SHAPES, ids=["x".join(map(str, s)) for s in SN_SHAPES])
@pytest.mark.parametrize("update", [1, 0], ids=["train", "eval"])
def test_sn_prepare(shape, update, pkg, device):
    C, KH, KW = shape
    K = C * KH * KW
    w = _randn((1, C, KH, KW), device, 130 + C) * 0.05
    w64 = w.double().reshape(-1)
    v0 = (w.reshape(-1) / w.norm() * 0.9 + _randn((K,), device, 131) * 0.01 / K ** 0.5).contiguous()
    u0 = -0.8
    u, v, sigma, wsn = _sn_run(pkg, w, u0, v0, C, KH, KW, update, device)
    L = _sn_depth(K)
    if update:
        # torch.nn.utils.spectral_norm, one power iteration: v = normalize(W^T u), u = normalize(W v), sigma = u . W v
        v64 = F.normalize(w64 * u0, dim=0, eps=1e-12)
        wv = (w64 * v64).sum()
        u64 = F.normalize(wv.reshape(1), dim=0, eps=1e-12)
        s64 = (u64 * wv).sum()
        assert u.item() == u64.item() == -1.0
        assert _worst((v.double() - v64).abs(), ((L + 3) / 2 + 4) * U * v64.abs() + 1e-300, "sn_prepare v") <= 1
        stol = (2 * L + 16) * U
    else:
        assert torch.equal(v, v0) and u.item() == torch.tensor(u0, dtype=torch.float32).item()
        u64 = torch.tensor(u0, dtype=torch.float32).double()
        s64 = u64 * (w64 * v0.double()).sum()
        stol = (L + 2) * U * abs(u64) * (w64 * v0.double()).abs().sum().item() / abs(s64.item()) + U
    assert _note("sn_prepare sigma", abs(sigma.double().item() - s64.item()) / (stol * abs(s64.item()))) <= 1
    ref = (w.double() / s64).reshape(C, KH, KW).permute(1, 2, 0).reshape(-1)         # (kh, kw, c)
    assert _worst((wsn.double() - ref).abs(), (stol + 2 * U) * ref.abs() + 1e-300, "sn_prepare wsn_k") <= 1


FM_CASES = [(1, 512, 16, 16), (8, 512, 16, 16), (16, 512, 16, 16), (8, 64, 4, 4), (16, 20, 3, 5)]


@pytest.mark.parametrize("case", FM_CASES, ids=["N{}_{}x{}x{}".format(*c) for c in FM_CASES])
def test_fullmap_conv(case, pkg, device):
    N, C, KH, KW = case
    K = C * KH * KW
    w = _randn((1, C, KH, KW), device, 140 + C) * 0.05
    u, v, sigma, wsn = _sn_run(pkg, w, 0.6, torch.zeros(K, device=device), C, KH, KW, 1, device)
    x = _randn((N, KH, KW, C), device, 141 + N)
    bias = torch.tensor([0.3], device=device)
    out = Out((N,), device)
    _call(pkg, "vcg_fullmap_fwd", P(x), P(wsn), P(bias), P(out.t), N, K, _st())
    g = _randn((N,), device, 142 + N)
    dx = Out((N, KH, KW, C), device)
    _call(pkg, "vcg_fullmap_dgrad", P(g), P(wsn), P(dx.t), N, K, _st())
    pre_w, pre_b = _randn((1, C, KH, KW), device, 143) * 1e-3, torch.tensor([0.25], device=device)
    gw, gb = Out((1, C, KH, KW), device, fill=pre_w), Out((1,), device, fill=pre_b)
    ws = _ws((K + 256) * 4, device)
    _call(pkg, "vcg_fullmap_wgrad", P(g), P(x), P(wsn), P(sigma), P(u), P(v), P(gw.t), P(gb.t), N, C, KH, KW, P(ws), ws.numel() * 4, _st())
    torch.cuda.synchronize()
    # float64 autograd of conv2d(x, W / sigma) + b, sigma = u . W v with u, v detached (they come from the power iteration)
    x64 = nchw(x).double().requires_grad_(True)
    W = w.double().requires_grad_(True)
    sig = u.double() * (W.reshape(1, -1) @ v.double())
    o = F.conv2d(x64, W / sig, bias.double()).reshape(-1)
    o.backward(g.double())
    L = _sn_depth(K)
    sg_tol = (2 * L + 16) * U                             # the kernel's sigma vs u . W v in float64 (test_sn_prepare)
    prod = (x64.detach().reshape(N, -1) * (W.detach() / sig.detach()).reshape(1, -1)).abs().sum(1)
    tol = (sg_tol + (L + 4) * U) * prod + U * (o.detach().abs() + 0.3)
    assert _worst((out.check("vcg_fullmap_fwd").double() - o.detach()).abs(), tol, "fullmap_fwd") <= 1
    dref = nhwc(x64.grad)
    assert _worst((dx.check("vcg_fullmap_dgrad").double() - dref).abs(), (sg_tol + 2 * U) * dref.abs() + 1e-300, "fullmap_dgrad") <= 1
    A = (g.double()[:, None, None, None] * x64.detach()).abs().sum(0, keepdim=True)     # sum_n |g_n x_nk|, NCHW (1, C, KH, KW)
    B = (A * W.detach().abs()).sum() / sig.detach().abs()
    scale = (A + B * (u.double() * v.double().reshape(1, C, KH, KW)).abs()) / sig.detach().abs()
    ref = pre_w.double() + W.grad
    tol = (N + L + sg_tol / U + 16) * U * scale + 2 * U * ref.abs()
    assert _worst((gw.check("vcg_fullmap_wgrad gw").double() - ref).abs(), tol + 1e-300, "fullmap_wgrad gw") <= 1
    bref = 0.25 + g.double().sum().item()
    assert abs(gb.check("vcg_fullmap_wgrad gbias").double().item() - bref) <= (N + 1) * U * (g.double().abs().sum().item() + 0.25 + abs(bref))
