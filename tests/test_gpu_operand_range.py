"""The operand scaling of the fp16 x 2 kernels (csrc/vcg_common.h: x / s = h + l, s a power of two from the tensor's largest
magnitude, "amax") beyond torch.randn: a wide range of magnitudes inside one tensor, degenerate tensors, and amax handles at the
end of their life.

1. Tiers.  run_conv_plan of test_gpu_conv_plans.py — every check of that file, its bounds unchanged — on make_operands(case, "tiers"):
   the randn draws times 2^-(Tn[n] + Tc[c]) (x), 2^-Tco[co] (w), 2^-(Tn'[n] + Tco'[co]) (dy), tiers cycling through
   0, 0, 9, 16, 19, 23, 30.  Operand elements land in every band of the split: h and l normal; h normal, l subnormal (more
   than 2^17 below amax); h subnormal (more than 2^28 below); nothing left (more than 2^40 below).  Here the floor F of that file's
   per-element bound binds: F = 2^-40 * 2 * Kred * amax_a * amax_b is what elements below 2^-17 of amax are allowed to lose.
   One case per fp16 x 2 family — tier_selection() picks, by the dispatch mirror and not by name, the case of CASES with the
   smallest reduction length that conv_plan maps to each family of TIER_REQUIRED; tests/test_host_logic.py checks without a GPU
   that every family is reached.  The vcg_conv_fwd_in_pre options are left out: that operand is normalised by construction.
2. What the bound can see (host only: tests/test_host_logic.py, test_operand_range_bound_rejects_broken_splits): emulate_gemm
   below is the documented arithmetic on a plain GEMM in float64 / fp32 on the CPU.  With tiered operands at the smallest and the
   largest reduction length of (1), the faithful emulation stays inside c_path U A + F and each of three broken ones leaves it:
   fp16 subnormals flushed, the low piece dropped below 2^-17 of amax, the scale of a Winograd-style operand (bounded by
   2^shift amax) one binade too small.  No family's case had to shrink: all three are rejected at the largest length, 4096 (the
   ring weight gradients, whose gate is a 64 x 64 map), with the 112 x 112 outputs the emulation uses (the smallest ring case
   writes 18432).  The third variant shows only as an fp16 overflow, and only when the operand comes within 2^-11 of its bound —
   the emulation plants one such element; randn data gets there by chance, so (1) promises nothing about an off-by-one shift
   beyond what its finite-output checks see.
3. Degenerate operands through four cases (direct split-operand, Winograd, slab + ring, thin-fold): dy = 0 (+0, and with -0), x = 0,
   x / dy entirely fp32-subnormal, x / dy in the low binades where vcg_scale_of clamps the exponent, one NaN, one +Inf, and a
   poisoned tensor whose handle comes from its producer (vcg_in_apply_h).
4. Handle lifetime: the last honoured and the first refused age, a slot really reused by another tensor, and ops.py across more
   than SLOTS - MARGIN library calls between forward and backward and between two blocks.  Out of scope and out of reach: the wrap
   of the 32-bit generation after 2^32 calls with its device-wide clear (misc.hip, vcg_amax_new).
"""
import ctypes
import struct

import pytest
import torch

from test_gpu_conv_plans import (CASES, FP16_DGRAD, FP16_FWD, LEAKY, NONE, RELU, U, _c_path, _reference, _relmax, case_desc, conv_plan,
                                 make_operands, run_conv_plan, tier_exponents, wino_T)
from test_gpu_norm_misc import AMAX_SHAPE, Out, P, _apply, _consumer_dgrad, _consumer_fwd, _randn, _st, _ws

pytestmark = pytest.mark.gpu


# ================================================================== 1. tiers: one case per fp16 x 2 family (host-only selection)
def tier_families(case):
    """{family: reduction length} — the fp16 x 2 kernel families a case reaches in its three directions, by the dispatch mirror"""
    pl = conv_plan(case_desc(case))
    g, f, d, w = pl["g"], pl["fwd"], pl["dgrad"], pl["wgrad"]
    out = {}
    fb, db, wb = f["branch"], d["branch"], w["branch"]
    if fb == "wino":
        out[f"fwd wino {f['kernel']}"] = g["kc"] * 9
    elif fb in FP16_FWD or (fb == "thin_fold" and f["kernel"]):
        out[f"fwd {fb}"] = g["K"]
    if db in FP16_DGRAD or (db == "thin_fold" and d["kernel"]):
        out[f"dgrad {db}"] = g["KH"] * g["KW"] * g["Cout"]
    if wb.startswith("wino"):
        out[f"wgrad {wb}"] = wino_T(g) * 16
        if "saved" in case[2]:
            out["wgrad wino saved"] = wino_T(g) * 16
    elif wb.startswith("ring"):
        out[f"wgrad {wb}"] = g["M"]
    elif w["kernel"] != "k_conv_wgrad<fp32 MFMA>":
        out[f"wgrad {w['kernel']}"] = g["M"]
    return out


TIER_REQUIRED = (
    [f"fwd {b}" for b in FP16_FWD if b != "wino"] + ["fwd thin_fold"]
    + [f"fwd wino {k}" for k in ("k_gemm_split<64, planes>", "k_gemm_split<128, planes>", "k_gemm_planes_dma")]
    + [f"dgrad {b}" for b in FP16_DGRAD] + ["dgrad thin_fold"]
    + ["wgrad wino_core", "wgrad wino_tr", "wgrad wino saved", "wgrad ring0", "wgrad ring1", "wgrad ring2",
       "wgrad k_conv_wgrad_split<64>", "wgrad k_conv_wgrad_split<128>"])


def tier_selection(cases=CASES):
    """{family: (reduction length, case)}: per family the case with the smallest reduction length (the first of equals)"""
    best = {}
    for c in cases:
        for fam, red in tier_families(c).items():
            if fam not in best or red < best[fam][0]:
                best[fam] = (red, c)
    return best


def tier_cases():
    sel = tier_selection()
    names = {c[0] for fam, (_, c) in sel.items() if fam in TIER_REQUIRED}
    return [c for c in CASES if c[0] in names]


TIER_CASES = tier_cases()


def test_tier_cases_reach_every_fp16_family():
    sel = tier_selection(TIER_CASES)
    missing = [f for f in TIER_REQUIRED if f not in sel]
    assert not missing, f"no tiered case reaches: {missing}"


@pytest.mark.parametrize("case", TIER_CASES, ids=[c[0] for c in TIER_CASES])
def test_tiered_operands_against_float64(case, pkg, device):
    run_conv_plan(case, pkg, device, "tiers")


# ================================================================== 2. the documented arithmetic on a plain GEMM (host only)
def scale_of(amax, shift=0):
    """vcg_scale_of (csrc/vcg_common.h) on the fp32 value `amax`"""
    bits = struct.unpack("<I", struct.pack("<f", amax))[0]
    e = (bits >> 23) & 0xFF
    f = 127 + shift if e in (0, 255) else e - 14 + shift
    return 2.0 ** (min(max(f, 1), 253) - 127)


def _split(x, s, amax, variant):
    xs = (x.double() / s).float()                       # a power of two: exact
    h = xs.half()
    l = (xs - h.float()).half()
    if variant == "flush":                              # fp16 subnormals flushed, in the conversion or in the MFMA
        h = torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)
        l = torch.where(l.abs() < 2.0 ** -14, torch.zeros_like(l), l)
    if variant == "drop_l":                             # the low piece of small elements never stored
        l = torch.where(x.abs() < 2.0 ** -17 * amax, torch.zeros_like(l), l)
    return h.double(), l.double()


def emulate_gemm(A, B, variant=None, a_shift=0, a_amax=None):
    """A [M, K] @ B [K, N] as the fp16 x 2 kernels compute it: s from vcg_scale_of, h = fp16(x / s), l = fp16(x / s - h), the
    products hh + hl + lh (exact in fp32) summed 16 k at a time into an fp32 accumulator, times sA sB.  `a_amax`, `a_shift`: A is
    a transformed tensor bounded by 2^a_shift * a_amax (the Winograd operands), scaled by that bound instead of its own amax."""
    aa, ab = A.abs().max().item(), B.abs().max().item()
    sa, sb = scale_of(aa if a_amax is None else a_amax, a_shift), scale_of(ab)
    ah, al = _split(A, sa, aa, variant)
    bh, bl = _split(B, sb, ab, variant)
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for k0 in range(0, A.shape[1], 16):
        sl = slice(k0, k0 + 16)
        for p, q in ((ah, bh), (ah, bl), (al, bh)):
            acc = (acc.double() + p[:, sl] @ q[sl]).float()
    return acc * torch.tensor(sa, dtype=torch.float32) * torch.tensor(sb, dtype=torch.float32)


def tiered_gemm_operands(M, K, N, seed):
    """A [M, K] like x (tiers on the row — the image — and on k — the channel), B [K, N] like w (tiers on the output channel)"""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(K, N, generator=g) * (2.0 / K) ** 0.5
    A *= torch.exp2(tier_exponents(M)[:, None] + tier_exponents(K)[None, :]).float()
    B *= torch.exp2(tier_exponents(N)[None, :]).float()
    return A, B


def gemm_bound(A, B):
    """test_gpu_conv_plans.py's per-element bound c_path U A + F for a K-long reduction with one partial"""
    K = A.shape[1]
    mag = A.double().abs() @ B.double().abs()
    return _c_path(True, K, 1) * U * mag + 2.0 ** -40 * 2 * K * A.abs().max().item() * B.abs().max().item()


# ================================================================== 3. degenerate operands (GPU)
def _degenerate_cases():
    """four small cases, by plan: a direct split-operand forward and data gradient, Winograd in all three directions, the LDS slab
    with a ring weight gradient, the thin-fold forward on the MFMA column kernel — of each the one with the fewest input elements"""
    want = {
        "direct": lambda f, d, w: f["branch"] in ("split64", "split128") and d["branch"].startswith("split<"),
        "wino": lambda f, d, w: f["branch"] == "wino" and d["branch"] == "wino" and w["branch"].startswith("wino"),
        "slab_ring": lambda f, d, w: f["branch"] == "slab" and d["branch"] == "slab" and w["branch"].startswith("ring"),
        "thin_fold": lambda f, d, w: f["branch"] == "thin_fold" and bool(f["kernel"]),
    }
    out = {}
    for c in CASES:
        pl = conv_plan(case_desc(c))
        g = pl["g"]
        size = g["N"] * g["H"] * g["W"] * g["Cin"]
        for key, ok in want.items():
            if ok(pl["fwd"], pl["dgrad"], pl["wgrad"]) and g["act"] in (NONE, RELU, LEAKY) and (key not in out or size < out[key][0]):
                out[key] = (size, c)
    assert sorted(out) == sorted(want), f"no case for {sorted(set(want) - set(out))}"
    return [out[k][1] for k in want]


DEGENERATE = _degenerate_cases()
DEG_IDS = ["direct", "wino", "slab_ring", "thin_fold"]


class _Conv:
    """a case's three directions through the C ABI on NaN-prefilled, guarded outputs, the operands replaceable per call"""

    def __init__(self, case, pkg, device):
        self.lib, self.nat, self.device, self.case = pkg._native.lib(), pkg._native, device, case
        self.cd = case_desc(case)
        self.plan = conv_plan(self.cd)
        self.g = self.plan["g"]
        self.x, self.wt, self.bias, self.dy, self.g0, self.gb0 = make_operands(case, "randn", device)
        self.has_dgrad = self.plan["dgrad"]["branch"] != "unsupported"
        buf = Out((self.lib.vcg_pack_weight_floats(self.cd),), device)
        self.nat.check(self.lib.vcg_pack_weight(P(self.wt), P(buf.t), self.cd, _st()), "vcg_pack_weight")
        self.wf = buf.t

    def act(self, t):
        return {NONE: lambda v: v, RELU: torch.relu, LEAKY: lambda v: torch.nn.functional.leaky_relu(v, 0.2)}[self.g["act"]](t)

    def fwd(self, x, handle=0):
        g, lib = self.g, self.lib
        y = Out((g["N"], g["Ho"], g["Wo"], g["Cout"]), self.device)
        ws = _ws(lib.vcg_conv_fwd_workspace(self.cd), self.device)
        lib.vcg_amax_hint(handle, 0)
        self.nat.check(lib.vcg_conv_fwd(P(x), P(self.wf), P(self.bias), P(y.t), self.cd, P(ws), ws.numel() * 4, _st()), "vcg_conv_fwd")
        torch.cuda.synchronize()
        return y.check("vcg_conv_fwd")

    def dgrad(self, dy, handle=0):
        g, lib = self.g, self.lib
        dx = Out((g["N"], g["H"], g["W"], g["Cin"]), self.device)
        ws = _ws(lib.vcg_conv_dgrad_workspace(self.cd), self.device)
        self.nat.check(lib.vcg_conv_dgrad_h(P(dy), P(self.wf), P(dx.t), self.cd, P(ws), ws.numel() * 4, handle, _st()), "vcg_conv_dgrad")
        torch.cuda.synchronize()
        return dx.check("vcg_conv_dgrad")

    def wgrad(self, x, dy):
        lib = self.lib
        gw = Out(tuple(self.wt.shape), self.device, fill=self.g0)
        gb = Out((self.g["cout_log"],), self.device, fill=self.gb0)
        ws = _ws(lib.vcg_conv_wgrad_workspace(self.cd), self.device)
        self.nat.check(lib.vcg_conv_wgrad_saved(P(x), P(dy), P(gw.t), P(gb.t), None, self.cd, P(ws), ws.numel() * 4, _st()),
                       "vcg_conv_wgrad")
        torch.cuda.synchronize()
        return gw.check("gw"), gb.check("gbias")

    def ref(self, x, dy, wt=None, bias=True):
        g = self.g
        return _reference(x, self.wt if wt is None else wt, self.bias if bias else None, dy, g, g["act"] if bias else NONE,
                          g["cin_log"], g["cout_log"], torch.float64, self.device)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _interior(t, c_log):
    """an interior element of an NHWC tensor, in a logical channel"""
    n, h, w, _ = t.shape
    return (n - 1, h // 2, w // 2, min(1, c_log - 1))


@pytest.mark.parametrize("case", DEGENERATE, ids=DEG_IDS)
def test_zero_operands(case, pkg, device):
    """dy == 0 (all +0, then with some -0): dx exactly zero, gw and gbias bitwise what they held.  x == 0: y == act(bias) exactly
    in the logical channels (0 in the pad channels), gw bitwise what it held."""
    cv = _Conv(case, pkg, device)
    g = cv.g
    for negz in (False, True):
        dy = torch.zeros_like(cv.dy)
        if negz:
            dy.view(-1)[::3] = -0.0
        if cv.has_dgrad:
            dx = cv.dgrad(dy)
            assert (dx == 0).all(), f"{case[0]}: dy == 0 (-0: {negz}) gives a nonzero data gradient"
        gw, gb = cv.wgrad(cv.x, dy)
        assert torch.equal(_bits(gw), _bits(cv.g0)), f"{case[0]}: dy == 0 (-0: {negz}) changed gw"
        assert torch.equal(_bits(gb), _bits(cv.gb0)), f"{case[0]}: dy == 0 (-0: {negz}) changed gbias"
    x0 = torch.zeros_like(cv.x)
    y = cv.fwd(x0)
    want = torch.zeros_like(y)
    want[..., :g["cout_log"]] = cv.act(cv.bias[:g["cout_log"]])
    assert torch.equal(y, want), f"{case[0]}: x == 0 does not give act(bias)"
    gw, _ = cv.wgrad(x0, cv.dy)
    assert torch.equal(_bits(gw), _bits(cv.g0)), f"{case[0]}: x == 0 changed gw"


def _subnormal_like(t, c_log, seed):
    """every logical element an fp32 subnormal of magnitude < 2^-127 (exponent field 0, 22 random mantissa bits, random sign)"""
    gen = torch.Generator(device=t.device).manual_seed(seed)
    bits = torch.randint(0, 1 << 22, t.shape, generator=gen, device=t.device, dtype=torch.int32)
    sign = torch.randint(0, 2, t.shape, generator=gen, device=t.device, dtype=torch.int32) << 31
    out = (bits | sign).view(torch.float32).clone()
    out[..., c_log:] = 0
    return out


def _amax(t):
    """the largest magnitude as the kernels see it (bit patterns: immune to a flush of subnormals in torch's abs / max)"""
    return (_bits(t) & 0x7FFFFFFF).max().view(torch.float32).double().item()


TINY = 2.0 ** -149      # the spacing of fp32 subnormals: an output down there carries up to that much rounding of its own


@pytest.mark.parametrize("case", DEGENERATE, ids=DEG_IDS)
def test_lowest_binades(case, pkg, device):
    """An operand entirely fp32-subnormal (vcg_scale_of: nothing to scale), and one with amax in [2^-125, 2^-113), where the
    exponent of s is clamped at 1 and the operand sits below [2^14, 2^15): every output finite; the subnormal tensor moves y
    from act(bias) (dx from 0) by at most Kred amax amax; the clamped one stays within the bound of test_gpu_conv_plans.py against
    float64, F from the measured amax (+ 2^-149: the rounding of an output that is itself subnormal)."""
    cv = _Conv(case, pkg, device)
    g, pf, pd = cv.g, cv.plan["fwd"], cv.plan["dgrad"]
    k, cin_log, cout_log = g["KH"], g["cin_log"], g["cout_log"]
    aw = _amax(cv.wt)
    wino_f, wino_d = pf["branch"] == "wino", pd["branch"] == "wino"
    kf = g["kc"] * 9 if wino_f else g["K"]
    kd = k * k * g["Cout"]
    bias_y = torch.zeros((g["N"], g["Ho"], g["Wo"], g["Cout"]), device=device)
    bias_y[..., :cout_log] = cv.act(cv.bias[:cout_log])
    # ---- entirely subnormal
    xs = _subnormal_like(cv.x, cin_log, 11)
    y = cv.fwd(xs)
    assert torch.isfinite(y).all(), f"{case[0]}: subnormal x: non-finite y"
    lim = kf * _amax(xs) * aw + TINY
    assert ((y.double() - bias_y.double()).abs() <= lim).all(), f"{case[0]}: subnormal x moves y by more than Kred amax amax"
    gw, _ = cv.wgrad(xs, cv.dy)
    assert torch.isfinite(gw).all(), f"{case[0]}: subnormal x: non-finite gw"
    if cv.has_dgrad:
        dys = _subnormal_like(cv.dy, cout_log, 12)
        dx = cv.dgrad(dys)
        assert torch.isfinite(dx).all(), f"{case[0]}: subnormal dy: non-finite dx"
        assert (dx.double().abs() <= 4 * kd * _amax(dys) * aw + TINY).all(), f"{case[0]}: subnormal dy: dx above 4 Kred amax amax"
    # ---- the clamp range
    xc = cv.x * 2.0 ** -122
    ax = _amax(xc)
    assert 2.0 ** -125 <= ax < 2.0 ** -113
    y = cv.fwd(xc)
    assert torch.isfinite(y).all(), f"{case[0]}: x in the clamp range: non-finite y"
    y64, _, _, _ = cv.ref(xc, cv.dy)
    Ay, _, _, _ = cv.ref(xc.abs(), cv.dy.abs(), wt=cv.wt.abs(), bias=False)
    fp16_f = pf["branch"] in FP16_FWD or (pf["branch"] == "thin_fold" and bool(pf["kernel"]))
    tol = (_c_path(fp16_f, kf, pf["nsplit"] + k, wino_f) * U * Ay + 2.0 ** -40 * 2 * kf * ax * aw * (16 if wino_f else 1)
           + 4 * U * y64.abs() + TINY)
    worst, i = _relmax(y, y64, tol)
    assert worst <= 1.0, f"{case[0]}: x in the clamp range: element {i} of y is {worst:.3g} x its bound"
    gw, _ = cv.wgrad(xc, cv.dy)
    assert torch.isfinite(gw).all(), f"{case[0]}: x in the clamp range: non-finite gw"
    if cv.has_dgrad:
        dyc = cv.dy * 2.0 ** -122
        ady = _amax(dyc)
        assert 2.0 ** -125 <= ady < 2.0 ** -113
        dx = cv.dgrad(dyc)
        assert torch.isfinite(dx).all(), f"{case[0]}: dy in the clamp range: non-finite dx"
        _, dx64, _, _ = cv.ref(cv.x, dyc)
        _, Adx, _, _ = cv.ref(cv.x.abs(), dyc.abs(), wt=cv.wt.abs(), bias=False)
        fp16_d = pd["branch"] in FP16_DGRAD or (pd["branch"] == "thin_fold" and bool(pd["kernel"]))
        tol = (_c_path(fp16_d, kd, pd["nsplit"] + 9, wino_d) * U * Adx + 2.0 ** -40 * 2 * 4 * kd * ady * aw * (16 if wino_d else 1)
               + TINY)
        worst, i = _relmax(dx, dx64, tol)
        assert worst <= 1.0, f"{case[0]}: dy in the clamp range: element {i} of dx is {worst:.3g} x its bound"


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", DEGENERATE, ids=DEG_IDS)
def test_one_poisoned_element_stays_poison(case, poison, pkg, device):
    """One NaN, one +Inf at an interior element of x (forward, weight gradient) and of dy (data and weight gradient): every output
    element whose float64 reference is non-finite is non-finite.  No claim about the elements that do not depend on the plant
    (the dependency mask: an indicator tensor through the same reference with all-ones weights)."""
    cv = _Conv(case, pkg, device)
    g = cv.g
    ones = torch.ones_like(cv.wt)

    def planted(t, c_log):
        p, ind = t.clone(), torch.zeros_like(t)
        spot = _interior(t, c_log)
        p[spot] = poison
        ind[spot] = 1.0
        return p, ind

    def claim(what, got, ref, dep):
        bad = ~torch.isfinite(ref)
        assert bad.any(), f"{case[0]}: {what}: the reference does not see the plant"
        assert not (bad & (dep == 0)).any(), f"{case[0]}: {what}: the reference is non-finite where nothing depends on the plant"
        lost = bad & torch.isfinite(got)
        assert not lost.any(), (f"{case[0]}: {what}: {int(lost.sum())} of {int(bad.sum())} poisoned elements came out finite, "
                                f"the first at flat index {int(lost.flatten().nonzero()[0])}")

    xp, xi = planted(cv.x, g["cin_log"])
    dyp, dyi = planted(cv.dy, g["cout_log"])
    y64, _, dw64, _ = cv.ref(xp, cv.dy)
    ydep, _, dwdep, _ = cv.ref(xi, cv.dy.abs(), wt=ones, bias=False)
    claim("forward", cv.fwd(xp), y64, ydep)
    claim("weight gradient, x poisoned", cv.wgrad(xp, cv.dy)[0], dw64, dwdep)
    _, dx64, dw64, _ = cv.ref(cv.x, dyp)
    _, dxdep, dwdep, _ = cv.ref(cv.x.abs(), dyi, wt=ones, bias=False)
    claim("weight gradient, dy poisoned", cv.wgrad(cv.x, dyp)[0], dw64, dwdep)
    if cv.has_dgrad:
        claim("data gradient", cv.dgrad(dyp), dx64, dxdep)


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", DEGENERATE, ids=DEG_IDS)
def test_poisoned_producer_hands_over_a_poisoned_handle(case, poison, pkg, device):
    """The plant arrives through vcg_in_apply_h (mean 0, rstd 1): the handle it publishes describes a poisoned tensor, and the
    forward that takes it gives bitwise what it gives when it measures the tensor itself."""
    cv = _Conv(case, pkg, device)
    N, H, W, C = cv.x.shape
    t = cv.x.clone()
    t[_interior(t, cv.g["cin_log"])] = poison
    out, h = _apply(pkg, t, torch.zeros((N, C), device=device), torch.ones((N, C), device=device), None, NONE, False, device)
    torch.cuda.synchronize()
    xin = out.check("vcg_in_apply")
    assert not torch.isfinite(xin).all() and h != 0 and pkg._native.lib().vcg_amax_valid(h)
    a, b = cv.fwd(xin, h), cv.fwd(xin, 0)
    assert not torch.isfinite(b).all()
    assert torch.equal(_bits(a), _bits(b)), f"{case[0]}: the forward differs between the producer's handle and a measured amax"


# ================================================================== 4. handle lifetime (GPU)
SLOTS, MARGIN = 16384, 6144         # VCG_AMAX_SLOTS, VCG_AMAX_MARGIN (csrc/misc.hip): a handle is honoured at ages < SLOTS - MARGIN
PLANT = 1.5 * 2.0 ** 20             # unique: with any amax but the true one (a decoy's, the 0 of a generation mismatch) fp16 overflows


def _gen_of(h):
    return h & 0xFFFFFFFF


class _Burner:
    def __init__(self, pkg, device):
        self.lib = pkg._native.lib()
        self.t = torch.ones(4, device=device)
        assert self.t.data_ptr() % 16 == 0

    def measure(self, t):
        h = self.lib.vcg_amax_measure(P(t), t.numel(), _st())
        assert h != 0 and (h >> 56) == 0xA5
        return h

    def burn(self, k):
        """k calls of vcg_amax_measure on a 4-float tensor: one generation each; the last handle"""
        h = prev = self.measure(self.t)
        for _ in range(k - 1):
            h = self.measure(self.t)
            assert (_gen_of(h) - _gen_of(prev)) & 0xFFFFFFFF == 1, "vcg_amax_measure did not take exactly one generation"
            prev = h
        return h

    def burn_until(self, gen):
        """burn until the generation counter stands at `gen` (the next call gets gen + 1)"""
        now = _gen_of(self.measure(self.t))
        left = (gen - now) & 0xFFFFFFFF
        assert left < 4 * SLOTS, "the counter is already past the target"
        if left:
            now = _gen_of(self.burn(left))
        assert now == gen & 0xFFFFFFFF


def _planted(device):
    x = _randn(AMAX_SHAPE, device, 90) * 0.5
    x.view(-1)[12345] = PLANT
    return x


def _consumers_ignore_or_honour(pkg, x, h, device, what):
    for consumer in (_consumer_fwd, _consumer_dgrad):
        a, b = consumer(pkg, x, device, h), consumer(pkg, x, device, 0)
        assert torch.isfinite(b).all()
        assert torch.isfinite(a).all() and torch.equal(_bits(a), _bits(b)), f"{what}: {consumer.__name__} differs from handle 0"


def test_handle_boundary(pkg, device):
    """h = measure(x) is valid while the generation counter is at most gen(h) + SLOTS - MARGIN - 1 and refused from the next
    generation on; some generations inside, both consumers take it and give bitwise the handle-0 result."""
    lib, b = pkg._native.lib(), _Burner(pkg, device)
    x = _planted(device)
    h = b.measure(x)
    g0 = _gen_of(h)
    b.burn_until(g0 + SLOTS - MARGIN - 64)
    assert lib.vcg_amax_valid(h) == 1
    _consumers_ignore_or_honour(pkg, x, h, device, "64 generations inside the boundary")
    b.burn_until(g0 + SLOTS - MARGIN - 1)
    assert lib.vcg_amax_valid(h) == 1, "the last honoured age, SLOTS - MARGIN - 1, is refused"
    b.burn(1)
    assert lib.vcg_amax_valid(h) == 0, "the first refused age, SLOTS - MARGIN, is honoured"
    _consumers_ignore_or_honour(pkg, x, h, device, "at the first refused age")


@pytest.mark.parametrize("age", [SLOTS - MARGIN, SLOTS - 1, SLOTS, SLOTS + 1, 2 * SLOTS])
def test_handle_of_a_reused_slot(age, pkg, device):
    """Burn until the next generation is gen(h) + age and take it with measure(decoy), amax 2^-3 (at ages SLOTS and 2 SLOTS the
    decoy lands in h's own slot): h is refused and both consumers, given h, are finite and bitwise the handle-0 result."""
    lib, b = pkg._native.lib(), _Burner(pkg, device)
    x = _planted(device)
    decoy = torch.full((64,), 2.0 ** -3, device=device)
    h = b.measure(x)
    b.burn_until(_gen_of(h) + age - 1)
    hd = b.measure(decoy)
    assert (_gen_of(hd) - _gen_of(h)) & 0xFFFFFFFF == age
    assert (_gen_of(hd) % SLOTS == _gen_of(h) % SLOTS) == (age % SLOTS == 0)
    assert lib.vcg_amax_valid(h) == 0
    _consumers_ignore_or_honour(pkg, x, h, device, f"age {age}")


def _two_blocks(pkg, device):
    """the graph of test_gpu_parity.test_amax_handles_change_no_bit_and_stale_ones_are_refused"""
    ops = pkg.ops
    torch.manual_seed(1)
    spec1 = ops.ConvSpec(32, 64, 3, 1, 1, True, 1, ops.ACT_RELU, True)
    spec2 = ops.ConvSpec(64, 64, 3, 1, 1, True, 1, ops.ACT_RELU, True)
    w1 = torch.nn.Parameter(torch.randn(64, 32, 3, 3, device=device) * 0.1)
    w2 = torch.nn.Parameter(torch.randn(64, 64, 3, 3, device=device) * 0.1)
    b1 = torch.nn.Parameter(torch.zeros(64, device=device))
    b2 = torch.nn.Parameter(torch.zeros(64, device=device))
    x0 = torch.randn(2, 32, 64, 64, device=device)

    def run(between_blocks=None, before_backward=None):
        for p_ in (w1, w2, b1, b2):
            p_.grad = None
        x = ops.to_nhwc(x0).requires_grad_(True)
        h1 = ops.conv_block(x, w1, b1, spec1)
        tag = getattr(h1, "_vcg_amax", None)
        if between_blocks:
            between_blocks()
        y = ops.conv_block(h1, w2, b2, spec2)
        tag2 = getattr(h1, "_vcg_amax", None)
        if before_backward:
            before_backward()
        y.backward(ops.to_nhwc(torch.ones_like(y) * 1e-3))
        return (y.detach().clone(), x.grad.clone(), w1.grad.clone(), w2.grad.clone()), tag, tag2

    return run


def test_ops_backward_after_the_handles_have_aged(pkg, device):
    """forward, more than SLOTS - MARGIN library calls, backward (a long validation loop, gradient accumulation): y, x.grad and
    both weight gradients bitwise those of the run without the gap"""
    run, b = _two_blocks(pkg, device), _Burner(pkg, device)
    base, tag, _ = run()
    assert tag and pkg._native.lib().vcg_amax_valid(tag[0])
    aged, _, _ = run(before_backward=lambda: b.burn(SLOTS - MARGIN + 64))
    for what, u, v in zip(("y", "x.grad", "w1.grad", "w2.grad"), base, aged):
        assert torch.isfinite(v).all() and torch.equal(_bits(u), _bits(v)), f"{what} changed when the handles aged before the backward"


def test_ops_tag_ages_between_two_blocks(pkg, device):
    """h1 = block1(x), more than SLOTS - MARGIN library calls, block2(h1): bitwise the result without the gap; afterwards h1
    carries a handle that is valid now — _amax_of dropped the old one and the block measured once and tagged again"""
    lib = pkg._native.lib()
    run, b = _two_blocks(pkg, device), _Burner(pkg, device)
    base, _, _ = run()
    aged, tag, tag2 = run(between_blocks=lambda: b.burn(SLOTS - MARGIN + 64))
    for what, u, v in zip(("y", "x.grad", "w1.grad", "w2.grad"), base, aged):
        assert torch.isfinite(v).all() and torch.equal(_bits(u), _bits(v)), f"{what} changed when the tag aged between the blocks"
    assert tag and tag2 and tag2[0] != tag[0], "the aged handle was kept"
    assert (_gen_of(tag2[0]) - _gen_of(tag[0])) & 0xFFFFFFFF > SLOTS - MARGIN
    assert lib.vcg_amax_valid(tag[0]) == 0 and lib.vcg_amax_valid(tag2[0]) == 1
