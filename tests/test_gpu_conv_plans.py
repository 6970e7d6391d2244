"""Every launch plan of the convolution entry points (csrc/conv_igemm.hip and the kernels it dispatches to in conv_wino.hip,
gemm_split.hip, conv_slab.hip, conv_ring.hip, conv_thin.hip, conv_thinin.hip), called through the C ABI and compared element by
element with float64.

conv_plan(cd) below mirrors the host-side dispatch in Python: which branch plan_fwd, plan_dgrad and plan_wgrad (the one chain per
direction that every size query and launch of conv_igemm.hip reads) choose for a descriptor, with the plan parameters that matter
(tile, K slices, stream-K parts, reduction kernel, whether the forward leaves the InstanceNorm partials itself).  It mirrors the
predicates and the cost models (gemm_plan, plan_dgrad's stride-2 re-plan, wgrad_plan, ring_plan, colsum_plan) and the layouts
(pack_layout, the workspaces) — no kernel.  tests/test_native_abi.py checks it against the sizes the library reports without a GPU (they
encode the K-slice, Winograd, slab, ring and thin choices) over the case list and a sweep of a few hundred geometries, and checks
that CASES below still reach every branch of this table:

  forward        thin-fold (kw folded into N: the 64 -> 3 7x7 head); thin (Cout == 4, not foldable: KW * 4 > 32); thinin (the 3 -> 64 4x4 s2
                 discriminator stem); Winograd with k_gemm_split<64 / 128, planes> and with k_gemm_planes_dma (>= 256 tile rows),
                 ups 1 and 2, reflect and zero padding, a ragged count of 256-row tiles; LDS slab with and without tile statistics;
                 k_conv_fwd_split<128> / <64> with and without tile statistics; the fp32 tiles <128,128,2,false>, <128,128>
                 (K > 2048), <128,64>, <64,128>, <64,64>, <128,32,1>; K slices + k_splitk_finish under each epilogue activation
                 and with cout_log < Cout
  fused IN       vcg_conv_fwd_in_pre with pre_act none / ReLU / LeakyReLU on ups 1 and ups 2 layers, reflect and zero, N >= 3
  data gradient  thin-fold (the 3 -> 64 7x7 stem); thin; Winograd over the padded domain (reflect fold, zero crop; with the DMA
                 GEMM); LDS slab; k_conv_dgrad_split<128,2>, <64,2>, <32,1>, <64,2,false> (no planes); fp32 tiles; stride-2 parity
                 classes with and without the batched re-plan (< 384 workgroups) and with K slices; K slices at stride 1;
                 dbl_mirror (reflect sources on both sides of a pixel: 3x3 on a 3-wide map, 7x7 pad 3 on maps 4..7)
  weight grad.   Winograd stream-K core and the transposed planes GEMM (vcg_wino_wgrad_tr_ok), each with and without `saved`;
                 ring modes 0 (also at ups 2), 1 and 2; swapped roles (Cout == 4 where the ring does not take it); stream-K tiles
                 <64,64>, split<64>, split<128> (<64,128> is a candidate of gemm_plan, not of wgrad_plan); <= 24 and > 24 parts (k_slab_sum); k_wgrad_scatter,
                 k_wgrad_scatter_swapped and k_wgrad_reduce; bias column sums with gbias given and NULL, and cout_log < Cout

Out of scope: anything under -DVCG_STAMP.

What each GPU case checks, for the forward, the forward with statistics, the data gradient and the weight gradient:
  * every element against a float64 reference of the same operation (reflect or zero padding, PixelUnshuffle folded in the
    channel order (c, i, j), stride, epilogue activation) — F.conv2d / autograd in float64 on the device;
  * every element written and nothing past the end: outputs are NaN-prefilled with a guard band of sentinel words
    (test_gpu_norm_misc.Out), workspaces and `saved` NaN-filled, so a partial that is read must have been written;
  * pad channels: y[..., cout_log:] is exactly 0; dx[..., cin_log:] is exactly 0 as well (the kernels write the
    adjoint of zero weight columns; include/vcg.h says so at vcg_conv_dgrad);
  * accumulation: gw and gbias start from a fixed random G0; gw - G0 is compared with the reference, with U |G0| added to the
    bound; gbias = NULL writes nothing;
  * the Wf claim: where vcg_conv_reads_wf(cd) == 0, a pack with cd[VCG_CD_PACK_FLAGS] = 1 (Wf left out, NaN there) gives
    bitwise the same forward, forward-with-statistics and data gradient as the full pack;
  * determinism: every call twice on fresh NaN buffers, bitwise equal;
  * branch witness: the device kernel the mirror predicts appears in vcg_profile_read's table (branches without a bracketed
    MFMA kernel — thin, scatter / reduce, column sums — are covered by the CPU mirror check).

Tolerances (U = 2^-24).  Per element |got - ref| <= c_path U A + F, where
  A  the float64 convolution of absolute values: |x| * |w| for y, the adjoint of |dy| * |w| for dx (reflect sources added),
     sum |x| |dy| for dw;
  F  the amax floor of csrc/vcg_common.h: an operand element more than 2^17 below its tensor's largest magnitude keeps an
     absolute error of 2^-40 of that magnitude, so F = 2^-40 * 2 * Kred * amax_a * amax_b (times 16 for Winograd's scaled
     operands);
  c_path = e_prod + 8 sqrt(depth): e_prod = 12 for the fp16 x 2 products (each operand split to 22 bits: 2^-22 = 4U apiece,
     plus the dropped lo*lo term, 4U), 2 for the fp32 kernels; depth = the number of fp32 additions in sequence: Kred / 16
     MFMA steps of an accumulator (Kred for the VALU / fp32 kernels) + the K-slice or stream-K partials summed after it + the
     reflect sources the data gradient folds.  8 sqrt(depth) is the probabilistic bound of Higham & Mary (SIAM J. Sci. Comput.
     41, 2019) with lambda = 8: it holds but with probability 2 n exp(-32) per sum, and it is what makes the bound tight
     enough to see a lost fp16 low piece (2^-12 of an element) where a worst-case depth * U bound at Kred = 9216 would not;
  Winograd: x 16 — the transformed operands grow by |B^T d B| <= 4 max|d| and the output transform sums 4 x 4 products of
     those (|A^T m A| <= 4 max|m| per row and column pair), against A of the direct convolution.
Whole tensor: relative L2 against float64 <= max(4 x the relative L2 of PyTorch-CPU fp32 on the same data, floor), the floor
1e-7 for the fp32 kernels and 2^-22 for the fp16 x 2 ones: their operands keep 22 bits, so a short sum (the weight gradient of a
4-pixel map) cannot come within 4x of PyTorch's fp32, whose products are exact to 24.
vcg_conv_fwd_in_pre: the reference input is pre_act((t_prev - mean) rstd) in float64 from the fp32 statistics handed in;
mean / rstd of y to the bounds of test_gpu_fullsize.test_conv_fwd_in_statistics_at_headline_size (1e-6 of std + |mean|, 3e-6).
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_norm_misc import Out, P, _st, _ws, norm_plan

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
EPS = torch.tensor(1e-5, dtype=torch.float32).item()
NONE, RELU, LEAKY, TANH, SIGMOID = 0, 1, 2, 3, 4
F4 = 4


# ================================================================== the dispatch mirror (host only)
def _cdiv(a, b):
    return (a + b - 1) // b


def geom(cd):
    """vcg_conv_geom: the descriptor's fields and what follows from them (no argument checks beyond what the plans need)."""
    g = dict(N=cd[0], H=cd[1], W=cd[2], Cin=cd[3], Cout=cd[4], KH=cd[5], KW=cd[6], stride=cd[7], pad=cd[8], reflect=cd[9],
             ups=cd[10], act=cd[11], cin_log=cd[12], cout_log=cd[13])
    g["Hl"], g["Wl"] = g["H"] // g["ups"], g["W"] // g["ups"]
    g["Ho"] = (g["Hl"] + 2 * g["pad"] - g["KH"]) // g["stride"] + 1
    g["Wo"] = (g["Wl"] + 2 * g["pad"] - g["KW"]) // g["stride"] + 1
    g["M"] = g["N"] * g["Ho"] * g["Wo"]
    g["taps"] = g["KH"] * g["KW"] * g["ups"] * g["ups"]
    g["K"] = g["taps"] * g["Cin"]
    g["kc"] = g["ups"] * g["ups"] * g["Cin"]
    return g


# ---- conv_thin.hip / conv_thinin.hip
def thin_fwd_ok(g):
    return (g["Cout"] == 4 and g["stride"] == 1 and g["ups"] == 1 and g["KH"] == g["KW"] and g["KH"] % 2 == 1 and g["Cin"] % 16 == 0
            and g["pad"] == g["KH"] // 2)


def thin_dgrad_ok(g):
    return (g["Cin"] == 4 and g["stride"] == 1 and g["ups"] == 1 and g["KH"] == g["KW"] and g["KH"] % 2 == 1 and g["Cout"] % 16 == 0
            and g["pad"] == g["KH"] // 2)


def thin_fold_ok(g):
    return thin_fwd_ok(g) and g["KW"] * 4 <= 32 and g["cout_log"] <= 3


def thin_fold_dgrad_ok(g):
    return thin_dgrad_ok(g) and g["KW"] * 4 <= 32 and g["cin_log"] <= 3


def slab_col_ok(kh, c):
    return kh == 7 and c % 32 == 0 and c <= 128


def _fold_planes_floats(kh, c):
    return kh * c * 32 if slab_col_ok(kh, c) else 0


def thinin_fwd_ok(g):
    disc = g["KH"] == 4 and g["KW"] == 4 and g["stride"] == 2 and g["pad"] == 1
    return (disc and g["ups"] == 1 and g["Cin"] == 4 and g["Cout"] == 64 and g["Ho"] % 16 == 0 and g["Wo"] % 16 == 0
            and (not g["reflect"] or (g["H"] > g["pad"] + 8 and g["W"] > g["pad"] + 8)))


# ---- conv_wino.hip (gates: forward 100, data gradient 80, weight gradient 128)
def wino_weight_ok(g):
    kc = g["kc"]
    return (g["KH"] == 3 and g["KW"] == 3 and g["stride"] == 1 and g["pad"] == 1 and kc >= 128 and g["Cout"] >= 64
            and g["Cout"] % 64 == 0 and kc % 64 == 0)


def wino_map_ok(g):
    return wino_weight_ok(g) and not (g["Ho"] < 4 or g["Wo"] < 4 or g["Ho"] % 2 or g["Wo"] % 2)


def wino_T(g):
    return g["N"] * (g["Ho"] // 2) * (g["Wo"] // 2)


def wino_fwd_ok(g):
    if not wino_map_ok(g):
        return False
    T, kc, co = wino_T(g), g["kc"], g["Cout"]
    if kc * co < 100 * (kc + co):
        return False
    return T * kc * 4 < 1 << 31 and T * co * 4 < 1 << 31 and T * kc * 16 < 1 << 32


def wino_wgrad_ok(g):
    kc, co = g["kc"], g["Cout"]
    return wino_fwd_ok(g) and kc % 128 == 0 and kc * co >= 128 * (kc + co)


def wino_wgrad_tr_ok(g):
    if not wino_wgrad_ok(g):
        return False
    kc, co, T = g["kc"], g["Cout"], wino_T(g)
    return (T % 32 == 0 and kc % 32 == 0 and co % 128 == 0 and kc >= 256 and _cdiv(kc, 256) * (co // 128) * 16 >= 192
            and 16 * kc * T * 2 < 1 << 32 and 16 * co * T * 2 < 1 << 32)


def wino_dgrad_ok(g):
    if not wino_map_ok(g):
        return False
    kc, co = g["kc"], g["Cout"]
    if kc * co < 80 * (kc + co):
        return False
    Tp = g["N"] * (g["Ho"] // 2 + 1) * (g["Wo"] // 2 + 1)
    return Tp * kc * 4 < 1 << 31 and Tp * co * 4 < 1 << 31 and Tp * co * 16 < 1 << 32


def wino_takes_fwd(g):
    return wino_weight_ok(g) and g["kc"] * g["Cout"] >= 100 * (g["kc"] + g["Cout"])


def wino_takes_dgrad(g):
    return wino_weight_ok(g) and g["kc"] * g["Cout"] >= 80 * (g["kc"] + g["Cout"])


def planes_gemm(rows, n):
    """vcg_gemm_planes_batched's kernel for `rows` x `n` outputs per batch"""
    bn = 128 if n % 128 == 0 else 64
    return "k_gemm_planes_dma" if bn == 128 and rows >= 256 else f"k_gemm_split<{bn}, planes>"


# ---- conv_slab.hip / conv_ring.hip
def _slab_geom_ok(g):
    return g["KH"] == 3 and g["KW"] == 3 and g["stride"] == 1 and g["pad"] == 1 and g["ups"] == 1 and g["Hl"] >= 3 and g["Wl"] >= 3


def slab_fwd_ok(g):
    return (_slab_geom_ok(g) and g["Cin"] % 32 == 0 and g["Cin"] <= 128 and g["Cout"] % 64 == 0 and g["Cout"] <= 128
            and g["Ho"] * g["Wo"] >= 64 * 64)


def slab_dgrad_ok(g):
    return (_slab_geom_ok(g) and g["Cout"] % 32 == 0 and g["Cout"] <= 128 and (g["Cin"] == 32 or g["Cin"] % 64 == 0)
            and g["Cin"] <= 128 and g["H"] * g["W"] >= 64 * 64)


def ring_mode(g):
    if g["stride"] != 1 or g["KH"] != g["KW"] or g["Ho"] * g["Wo"] < 64 * 64 or g["Ho"] != g["Hl"] or g["Wo"] != g["Wl"]:
        return -1
    if g["KH"] == 3 and g["pad"] == 1 and g["Cin"] % 32 == 0 and g["kc"] <= 256 and g["Cout"] % 64 == 0 and g["Cout"] <= 256:
        return 0
    if g["ups"] != 1:
        return -1
    if g["KH"] == 7 and g["pad"] == 3 and g["reflect"] and g["Cin"] == 4 and g["Cout"] == 64:
        return 1
    if g["KH"] == 7 and g["pad"] == 3 and g["reflect"] and g["Cin"] == 64 and g["Cout"] == 4:
        return 2
    return -1


def ring_plan(g):
    mode = ring_mode(g)
    yd, xd = (g["H"] + 6, g["W"] + 6) if mode == 2 else (g["Ho"], g["Wo"])
    nseg = _cdiv(xd, 32)
    sub = (g["Cout"] // 64) * (g["kc"] // 32) if mode == 0 else 1
    nrs = max(768 // (g["N"] * nseg * sub), 1)
    rows = max(_cdiv(yd, nrs), 8)
    nrs = _cdiv(yd, rows)
    nwg = g["N"] * nseg * nrs
    per = _cdiv(nwg, 16)
    return dict(mode=mode, sub=sub, nseg=nseg, rows=rows, nrs=nrs, nwg=nwg, NR=(9 if mode == 0 else 7) * 32, G=_cdiv(nwg, per),
                ragged_rows=yd % rows != 0, ragged_seg=xd % 32 != 0)


# ---- conv_igemm.hip
def wft_wanted(g):
    return g["Cout"] >= 64 and g["Cin"] % 4 == 0 and not wino_takes_fwd(g)


def wfd_wanted(g):
    return (g["Cout"] >= 64 and g["Cout"] % 32 == 0 and not wino_takes_dgrad(g) and not thin_fold_dgrad_ok(g)
            and not thin_dgrad_ok(g))


def fwd_slab_ok(g):
    return not thin_fold_ok(g) and not thin_fwd_ok(g) and not wino_fwd_ok(g) and wft_wanted(g) and slab_fwd_ok(g)


def dgrad_slab_ok(g):
    return (not thin_fold_dgrad_ok(g) and not thin_dgrad_ok(g) and not wino_dgrad_ok(g) and wfd_wanted(g)
            and slab_dgrad_ok(g))


def gemm_plan(rows, cols, nkt, allow_split, batches=1, allow_bn32=False, single_level=False):
    """(bm, bn, nsplit, kt_per): the forward / data-gradient tile and K-slice cost model"""
    cands = [(128, 128, 3 if single_level else 2, 5.4 if single_level else 5.1), (128, 64, 3, 4.7), (64, 128, 3, 4.7),
             (64, 64, 4, 4.8), (128, 32, 4, 3.6)]
    best, out = 1e30, (64, 64, 1, nkt)
    for bm, bn, res, t_step in cands:
        if bn == 32 and not (allow_bn32 and cols <= 32):
            continue
        if bn == 128 and cols <= 64:
            continue
        if bm == 128 and rows <= 64:
            continue
        tiles = _cdiv(rows, bm) * _cdiv(cols, bn) * batches
        slots = 256 * res
        for ns in range(1, (32 if allow_split else 1) + 1):
            kt = _cdiv(nkt, ns)
            if ns > 1 and kt < 8:
                break
            real_ns = _cdiv(nkt, kt)
            rounds = _cdiv(tiles * real_ns, slots)
            t = float(rounds * kt) * t_step * 1.0
            if real_ns > 1:
                t += float(real_ns) * rows * cols * 8.0 / 3.0e6 + 3.0
            if t < best * 0.97:
                best, out = t, (bm, bn, real_ns, kt)
    return out


def fwd_plan(g):
    return gemm_plan(g["M"], g["Cout"], _cdiv(g["K"], 32), True, 1, True)


def dgrad_setup(g):
    """(bm, bn, nsplit, kt_per, batched re-plan taken)"""
    s = g["stride"]
    mc = g["N"] * (g["Hl"] // s) * (g["Wl"] // s)
    nb = g["kc"]
    bm, bn, ns, kt = gemm_plan(mc, nb, _cdiv(g["KH"] * g["KW"] * g["Cout"], 32), s == 1, 1, True)
    replan = False
    if s > 1 and g["KH"] % s == 0 and g["KW"] % s == 0:
        wgs = _cdiv(mc, bm) * _cdiv(nb, bn) * s * s
        if wgs < 384:
            replan = True
            bm, bn, ns, kt = gemm_plan(mc, nb, _cdiv((g["KH"] // s) * (g["KW"] // s) * g["Cout"], 32), True, s * s, True)
    return bm, bn, ns, kt, replan


def wgrad_plan(g, batches=1):
    """(bm, bn, grid, len, parts) of the stream-K weight gradient (bm = 256 only in the diagnostic build)"""
    total = _cdiv(g["M"], 32)
    best, out = 1e30, None
    for bm, bn, res, t_step in [(128, 128, 2, 5.1), (128, 64, 3, 4.7), (64, 64, 5, 4.8)]:
        if bn == 128 and g["Cout"] <= 64:
            continue
        if bm >= 128 and g["K"] <= 64:
            continue
        if batches > 1 and g["K"] % bm:
            continue
        ntr, ntn = _cdiv(g["K"], bm) * batches, _cdiv(g["Cout"], bn)
        tiles = ntr * ntn
        units = tiles * total
        if units >= 1 << 30:
            continue
        slots = 256 * res
        ln = _cdiv(units, slots)
        if ln < 8:
            ln = units if units < 8 else 8
        grid = _cdiv(units, ln)
        parts = _cdiv(total, ln) + 1
        t = float(ln) * t_step + float(grid + tiles) * bm * bn * 8.0 / 3.0e6
        if t < best * 0.97:
            best, out = t, dict(bm=bm, bn=bn, grid=grid, len=ln, parts=parts, total=total)
    return out


def colsum_plan(g):
    c4 = g["Cout"] // 4
    tc = 1
    while tc * 2 <= c4 and tc * 2 <= 256:
        tc *= 2
    cgroups = _cdiv(c4, tc)
    tp = 256 // tc
    want = max(512 // cgroups, 1)
    rows = max(_cdiv(g["M"], want), 4 * tp)
    return dict(tc=tc, cgroups=cgroups, rows=rows, nchunk=_cdiv(g["M"], rows))


def wgrad_swapped_ok(g):
    return g["Cout"] == 4 and g["stride"] == 1 and g["ups"] == 1 and g["Ho"] == g["H"] and g["Wo"] == g["W"] and g["Cin"] >= 32


def swapped_geom(g):
    s = dict(g)
    s.update(Cin=4, Cout=g["Cin"], cin_log=g["cout_log"], cout_log=g["cin_log"], taps=g["KH"] * g["KW"], M=g["N"] * g["H"] * g["W"],
             act=0)
    s["K"] = s["taps"] * 4
    s["kc"] = 4
    return s


def wino_gemm_geom(g, T):
    return dict(N=1, H=1, W=T, Cin=g["kc"], Cout=g["Cout"], KH=1, KW=1, K=g["kc"], M=T, kc=g["kc"])


def _stream_k_kernel(bm, bn):
    return ("k_conv_wgrad_split<128>" if bn == 128 else "k_conv_wgrad_split<64>") if bm == 128 else "k_conv_wgrad<fp32 MFMA>"


def _fwd_fp32_kernel(bm, bn, K):
    if bn == 32:
        return "fp32<128,32,1>"
    if bm == 128 and bn == 128 and K <= 2048:
        return "fp32<128,128,2,false>"
    return f"fp32<{bm},{bn}>"


def conv_plan(cd):
    """The branch each direction takes for descriptor cd, with its plan parameters and the device kernel the profile table
    names for it (None: the branch launches no bracketed MFMA kernel of its own)."""
    g = geom(cd)
    # ---------------------------------------------------------------- forward (plan_fwd)
    if thin_fold_ok(g):
        fwd = dict(branch="thin_fold", stats="pass", kernel="k_conv_slab<4, 1, 7, 1>" if slab_col_ok(g["KH"], g["Cin"]) else None)
    elif thin_fwd_ok(g):
        fwd = dict(branch="thin", stats="pass", kernel=None)
    elif thinin_fwd_ok(g):
        fwd = dict(branch="thinin", stats="fused", kernel=f"k_conv_thinin<{g['KH']}, {g['KW']}, {g['stride']}>")
    elif wino_fwd_ok(g):
        T = wino_T(g)
        fwd = dict(branch="wino", stats="fused", kernel=planes_gemm(T, g["Cout"]), rows=T, ragged=T % 256 != 0)
    elif fwd_slab_ok(g):
        st = g["Ho"] % 8 == 0 and g["Wo"] % 16 == 0
        fwd = dict(branch="slab", stats="fused" if st else "pass", kernel="k_conv_slab<2, 2, 3, 3>")
    else:
        bm, bn, ns, kt = fwd_plan(g)
        if bm == 128 and bn >= 64 and wft_wanted(g):
            tile_stats = ns == 1 and (g["Ho"] * g["Wo"]) % 128 == 0
            fwd = dict(branch=f"split{bn}", stats="fused" if tile_stats else "pass", kernel=f"k_conv_fwd_split<{bn}>")
        else:
            fwd = dict(branch=_fwd_fp32_kernel(bm, bn, g["K"]), stats="pass", kernel="k_conv_fwd<fp32 MFMA>")
        fwd.update(bm=bm, bn=bn, nsplit=ns, kt_per=kt)
    fwd.setdefault("nsplit", 1)
    fwd["pre_ok"] = not thin_fold_ok(g) and not thin_fwd_ok(g) and wino_fwd_ok(g)
    # ---------------------------------------------------------------- data gradient (plan_dgrad)
    s = g["stride"]
    if g["Hl"] % s or g["Wl"] % s:
        dg = dict(branch="unsupported", kernel=None)
    elif thin_fold_dgrad_ok(g):
        dg = dict(branch="thin_fold", kernel="k_conv_slab<4, 1, 7, 1>" if slab_col_ok(g["KH"], g["Cout"]) else None)
    elif thin_dgrad_ok(g):
        dg = dict(branch="thin", kernel=None)
    elif wino_dgrad_ok(g):
        Tp = g["N"] * (g["Ho"] // 2 + 1) * (g["Wo"] // 2 + 1)
        dg = dict(branch="wino", kernel=planes_gemm(Tp, g["kc"]), fold="reflect" if g["reflect"] else "crop")
    elif dgrad_slab_ok(g):
        dg = dict(branch="slab", kernel="k_conv_slab<4, 1, 3, 3>" if g["Cin"] == 32 else "k_conv_slab<2, 2, 3, 3>")
    else:
        bm, bn, ns, kt, replan = dgrad_setup(g)
        planes = bm == 128 and bn >= 64 and wfd_wanted(g)
        nopl64 = not planes and bm == 128 and bn == 64
        if planes:
            br, kern = f"split<{bn},2>", f"k_conv_dgrad_split<{bn}, 2>"
        elif bn == 32:
            br, kern = "split<32,1>", "k_conv_dgrad_split<32, 1>"
        elif nopl64:
            br, kern = "split<64,2,false>", "k_conv_dgrad_split<64, 2>"
        else:
            br, kern = f"fp32<{bm},{bn}>", "k_conv_dgrad<fp32 MFMA>"

        def dbl(L):
            return max(1, L - 1 - g["pad"]) <= min(g["pad"], L - 2)
        dg = dict(branch=br, kernel=kern, bm=bm, bn=bn, nsplit=ns, kt_per=kt, replan=replan,
                  dbl_mirror=bool(g["reflect"] and (dbl(g["Hl"]) or dbl(g["Wl"]))))
    dg.setdefault("nsplit", 1)
    # ---------------------------------------------------------------- weight gradient (plan_wgrad)
    if wino_wgrad_ok(g):
        T = wino_T(g)
        if wino_wgrad_tr_ok(g):
            wg = dict(branch="wino_tr", kernel=planes_gemm(g["kc"], g["Cout"]), parts=1)
        else:
            wp = wgrad_plan(wino_gemm_geom(g, T), 16)
            wg = dict(branch="wino_core", kernel=_stream_k_kernel(wp["bm"], wp["bn"]), parts=wp["parts"], bm=wp["bm"], bn=wp["bn"])
    elif ring_mode(g) >= 0:
        rp = ring_plan(g)
        wg = dict(branch=f"ring{rp['mode']}", kernel="k_wgrad_ring<false>" if rp["mode"] == 0 else "k_wgrad_ring<true>",
                  ragged=rp["ragged_rows"] or rp["ragged_seg"], parts=rp["nwg"])
    else:
        swapped = wgrad_swapped_ok(g)
        q = swapped_geom(g) if swapped else g
        wp = wgrad_plan(q)
        T = q["KH"] * q["KW"] * q["ups"] * q["ups"]
        totalw = q["K"] * q["Cout"]
        red = ("scatter_swapped" if swapped else "scatter" if totalw < 1 << 20 or T * 8 * 33 * 4 > 64 * 1024 else "reduce")
        wg = dict(branch="swapped" if swapped else "stream_k", kernel=_stream_k_kernel(wp["bm"], wp["bn"]),
                  tile=f"<{wp['bm']},{wp['bn']}>", parts=wp["parts"], slab_sum=wp["parts"] > 24, reduce=red)
    return dict(g=g, fwd=fwd, dgrad=dg, wgrad=wg)


# ---- the sizes the library reports for a descriptor (what test_native_abi.py compares with the library)
def _wf_floats(g):
    return _cdiv(g["K"] * g["Cout"], 64) * 64


def pack_weight_floats(g):
    wino_u = 16 * g["kc"] * g["Cout"]
    n = _wf_floats(g)
    n += wino_u if wino_takes_fwd(g) else 0
    n += wino_u if wino_takes_dgrad(g) else 0
    n += g["KH"] * g["Cin"] * 32 + _fold_planes_floats(g["KH"], g["Cin"]) if thin_fold_ok(g) else 0
    n += g["KH"] * g["Cout"] * 32 + _fold_planes_floats(g["KH"], g["Cout"]) if thin_fold_dgrad_ok(g) else 0
    n += g["Cout"] * _cdiv(g["K"], 32) * 32 if wft_wanted(g) else 0
    n += g["KH"] * g["KW"] * g["kc"] * (g["Cout"] // 32) * 32 if wfd_wanted(g) else 0
    return n + 16


def _thin_fold_ws(N, Ho, Wpad):
    return N * Ho * Wpad * 32 * F4 + 256


def fwd_workspace(g):
    if thin_fold_ok(g):
        return _thin_fold_ws(g["N"], g["Ho"], g["W"] + 2 * g["pad"])
    if thin_fwd_ok(g) or thinin_fwd_ok(g):
        return 0
    if wino_fwd_ok(g):
        return 16 * wino_T(g) * (g["kc"] + g["Cout"]) * F4 + 512
    if fwd_slab_ok(g):
        return 0
    _, _, ns, _ = fwd_plan(g)
    return ns * g["M"] * g["Cout"] * F4 + 256 if ns > 1 else 0


def dgrad_workspace(g):
    if g["Hl"] % g["stride"] or g["Wl"] % g["stride"]:
        return 0
    thin_ws = g["N"] * (g["H"] + 2 * g["pad"]) * (g["W"] + 2 * g["pad"]) * 4 * F4 + 256
    if thin_fold_dgrad_ok(g):
        return thin_ws + 256 + _thin_fold_ws(g["N"], g["H"] + 2 * g["pad"], g["Wo"] + 4 * g["pad"])
    if thin_dgrad_ok(g):
        return thin_ws
    if wino_dgrad_ok(g):
        return 16 * g["N"] * (g["Ho"] // 2 + 1) * (g["Wo"] // 2 + 1) * (g["kc"] + g["Cout"]) * F4 + 1024
    if dgrad_slab_ok(g):
        return g["N"] * (g["H"] + 2) * (g["W"] + 2) * g["Cin"] * F4 + 256
    _, _, ns, _, _ = dgrad_setup(g)
    return ns * g["N"] * g["H"] * g["W"] * g["Cin"] * F4 + 256 if ns > 1 else 0


def wgrad_workspace(g):
    cols = colsum_plan(g)["nchunk"] * g["Cout"] * F4
    if wino_wgrad_ok(g):
        T = wino_T(g)
        core = wgrad_plan(wino_gemm_geom(g, T), 16)["parts"] * 16 * g["kc"] * g["Cout"] * F4 + 256
        return _cdiv(16 * T * (g["kc"] + g["Cout"]) * F4 + 512 + core, 256) * 256 + cols + 1024
    if ring_mode(g) >= 0:
        rp = ring_plan(g)
        ring = (rp["sub"] * rp["nwg"] + rp["sub"] * rp["G"]) * rp["NR"] * 64 * F4 + 256
        return _cdiv(ring, 256) * 256 + cols + 1024
    q = swapped_geom(g) if wgrad_swapped_ok(g) else g
    wp = wgrad_plan(q)
    return wp["parts"] * q["K"] * q["Cout"] * F4 + 16 * q["K"] * q["Cout"] * F4 + cols + 1024


def reads_wf(g):
    if thin_fold_ok(g):
        f = False
    elif thin_fwd_ok(g) or thinin_fwd_ok(g):
        f = True
    elif wino_fwd_ok(g) or fwd_slab_ok(g):
        f = False
    else:
        bm, bn, _, _ = fwd_plan(g)
        f = not (bm == 128 and bn >= 64 and wft_wanted(g))
    if f:
        return 1
    if g["Hl"] % g["stride"] or g["Wl"] % g["stride"]:
        return 1
    if thin_fold_dgrad_ok(g):
        return 0
    if thin_dgrad_ok(g):
        return 1
    if wino_dgrad_ok(g) or dgrad_slab_ok(g):
        return 0
    bm, bn, _, _, _ = dgrad_setup(g)
    return 0 if (bm == 128 and bn >= 64 and wfd_wanted(g)) else 1


def saved_floats(g):
    return 16 * wino_T(g) * g["kc"] + 16 if wino_wgrad_ok(g) else 0


def fwd_tile_stats(g):
    """the direct split-operand forward leaves the partials itself: every 128-row tile inside one image, no K slices"""
    if thin_fold_ok(g) or thin_fwd_ok(g) or thinin_fwd_ok(g) or wino_fwd_ok(g) or fwd_slab_ok(g):
        return False
    bm, bn, ns, _ = fwd_plan(g)
    return bm == 128 and bn >= 64 and ns == 1 and wft_wanted(g) and (g["Ho"] * g["Wo"]) % 128 == 0


def fwd_in_workspace(g):
    """vcg_conv_fwd_in_workspace: the conv workspace rounded up to 256 bytes, then the InstanceNorm partials of whoever leaves them
    (16 bytes per (image, chunk, channel): a double sum and a double sum of squares) or the workspace of the separate pass"""
    N, HoWo, co = g["N"], g["Ho"] * g["Wo"], g["Cout"]
    if not thin_fold_ok(g) and not thin_fwd_ok(g) and thinin_fwd_ok(g):
        part = N * (g["Ho"] // 16) * (g["Wo"] // 16) * co * 16
    elif wino_fwd_ok(g):
        part = N * norm_plan(N, (g["Ho"] // 2) * (g["Wo"] // 2), co)["nchunk"] * co * 16
    elif fwd_slab_ok(g) and g["Ho"] % 8 == 0 and g["Wo"] % 16 == 0:
        part = N * (g["Ho"] // 8) * (g["Wo"] // 16) * co * 16
    elif fwd_tile_stats(g):
        part = N * (HoWo // 128) * co * 16
    else:
        part = N * norm_plan(N, HoWo, co)["nchunk"] * co * 20 + N * co * 8 + 512          # vcg_in_workspace
    return _cdiv(fwd_workspace(g), 256) * 256 + part


def library_sizes(lib, cd):
    return dict(fwd_ws=lib.vcg_conv_fwd_workspace(cd), fwd_in_ws=lib.vcg_conv_fwd_in_workspace(cd),
                dgrad_ws=lib.vcg_conv_dgrad_workspace(cd),
                wgrad_ws=lib.vcg_conv_wgrad_workspace(cd), pack=lib.vcg_pack_weight_floats(cd), reads_wf=lib.vcg_conv_reads_wf(cd),
                saved=lib.vcg_conv_saved_floats(cd), pre_ok=lib.vcg_conv_pre_ok(cd))


def mirror_sizes(cd):
    g = geom(cd)
    return dict(fwd_ws=fwd_workspace(g), fwd_in_ws=fwd_in_workspace(g), dgrad_ws=dgrad_workspace(g), wgrad_ws=wgrad_workspace(g),
                pack=pack_weight_floats(g), reads_wf=reads_wf(g), saved=saved_floats(g), pre_ok=int(conv_plan(cd)["fwd"]["pre_ok"]))


def desc(n, h, w, cin, cout, k, stride=1, pad=1, reflect=1, ups=1, act=0, cin_log=None, cout_log=None):
    cd = (ctypes.c_int32 * 16)()
    cd[0:14] = [n, h, w, cin, cout, k, k, stride, pad, reflect, ups, act, cin_log or cin, cout_log or cout]
    return cd


# ---- the branch table: what a case reaches
def branch_labels(cd, opts=()):
    """The rows of the module docstring's table that a case (descriptor + test options) reaches, by the mirror."""
    pl = conv_plan(cd)
    g, f, d, w = pl["g"], pl["fwd"], pl["dgrad"], pl["wgrad"]
    out = set()
    fb = f["branch"]
    out.add(f"fwd {fb}")
    if fb == "wino":
        out.add(f"fwd wino {f['kernel']}")
        out.add(f"fwd wino ups{g['ups']}")
        out.add("fwd wino reflect" if g["reflect"] else "fwd wino zero")
        if f["ragged"]:
            out.add("fwd wino ragged 256-row tiles")
    if fb in ("slab", "split64", "split128"):
        out.add(f"fwd {fb} stats {f['stats']}")
    if f["nsplit"] > 1:
        out.add(f"fwd K slices act{g['act']}")
        if g["cout_log"] < g["Cout"]:
            out.add("fwd K slices cout_log < Cout")
    for a in opts_pre(opts):
        if f["pre_ok"] and g["N"] >= 3:
            out.add(f"fwd_in_pre act{a} ups{g['ups']} {'reflect' if g['reflect'] else 'zero'}")
    db = d["branch"]
    out.add(f"dgrad {db}")
    if db == "wino":
        out.add(f"dgrad wino {d['fold']}")
        out.add(f"dgrad wino {d['kernel']}")
    if "bm" in d:
        if g["stride"] == 2:
            out.add("dgrad stride 2 batched re-plan" if d["replan"] else "dgrad stride 2 plain plan")
            if d["nsplit"] > 1:
                out.add("dgrad stride 2 K slices")
        elif d["nsplit"] > 1:
            out.add("dgrad K slices")
        if d["dbl_mirror"]:
            out.add(f"dgrad dbl_mirror k{g['KH']}")
    wb = w["branch"]
    out.add(f"wgrad {wb}")
    if wb.startswith("wino"):
        out.add(f"wgrad {wb} {'saved' if 'saved' in opts else 'recomputed'}")
    if wb == "ring0" and g["ups"] == 2:
        out.add("wgrad ring0 ups2")
    if wb in ("stream_k", "swapped"):
        out.add(f"wgrad tile {w['kernel'] if w['kernel'] != 'k_conv_wgrad<fp32 MFMA>' else w['tile']}")
        out.add("wgrad parts > 24 (k_slab_sum)" if w["slab_sum"] else "wgrad parts <= 24")
        out.add(f"wgrad {w['reduce']}")
    out.add("wgrad gbias NULL" if "gbias_null" in opts else "wgrad gbias")
    if g["cout_log"] < g["Cout"] and "gbias_null" not in opts:
        out.add("wgrad gbias cout_log < Cout")
    return out


def opts_pre(opts):
    return [int(o[3:]) for o in opts if o.startswith("pre")]


REQUIRED = (
    ["fwd thin_fold", "fwd thin", "fwd thinin", "fwd wino k_gemm_planes_dma", "fwd wino ups1", "fwd wino ups2",
     "fwd wino reflect", "fwd wino zero", "fwd wino ragged 256-row tiles", "fwd slab stats fused", "fwd slab stats pass",
     "fwd split128 stats fused", "fwd split128 stats pass", "fwd split64 stats fused", "fwd split64 stats pass",
     "fwd fp32<128,128,2,false>", "fwd fp32<128,128>", "fwd fp32<128,64>", "fwd fp32<64,128>", "fwd fp32<64,64>",
     "fwd fp32<128,32,1>", "fwd K slices cout_log < Cout"]
    + [f"fwd wino k_gemm_split<{bn}, planes>" for bn in (64, 128)]
    + [f"fwd K slices act{a}" for a in (NONE, RELU, LEAKY, TANH, SIGMOID)]
    + [f"fwd_in_pre act{a} ups{u} {p}" for a in (NONE, RELU, LEAKY) for u in (1, 2) for p in ("reflect", "zero")]
    + ["dgrad thin_fold", "dgrad thin", "dgrad wino reflect", "dgrad wino crop", "dgrad wino k_gemm_planes_dma", "dgrad slab",
       "dgrad split<128,2>", "dgrad split<64,2>", "dgrad split<32,1>", "dgrad split<64,2,false>", "dgrad stride 2 plain plan",
       "dgrad stride 2 batched re-plan", "dgrad stride 2 K slices", "dgrad K slices", "dgrad dbl_mirror k3", "dgrad dbl_mirror k7"]
    + ["wgrad wino_core recomputed", "wgrad wino_core saved", "wgrad wino_tr recomputed", "wgrad wino_tr saved", "wgrad ring0",
       "wgrad ring0 ups2", "wgrad ring1", "wgrad ring2", "wgrad swapped", "wgrad tile <64,64>", "wgrad tile k_conv_wgrad_split<64>",
       "wgrad tile k_conv_wgrad_split<128>", "wgrad parts <= 24", "wgrad parts > 24 (k_slab_sum)", "wgrad scatter",
       "wgrad scatter_swapped", "wgrad reduce", "wgrad gbias", "wgrad gbias NULL", "wgrad gbias cout_log < Cout"])


# ================================================================== the case list
def C(name, n, h, cin, cout, k, s=1, pad=None, reflect=1, ups=1, act=NONE, cin_log=None, cout_log=None, w=None, opts=()):
    pad = (k - 1) // 2 if pad is None else pad
    return (name, (n, h, h if w is None else w, cin, cout, k, s, pad, reflect, ups, act, cin_log, cout_log), tuple(opts))


# each one chosen for a branch of the table (test_native_abi.py checks that they still reach them: the training sizes do not
# reach most of them); the smallest geometry that does
CASES = [
    # ---- thin layers
    C("head 64->3 k7 (thin-fold + slab column kernel), ring mode 2", 1, 64, 64, 4, 7, cout_log=3),
    C("head 64->3 k7 on a small map (swapped roles), gbias NULL", 2, 12, 64, 4, 7, cout_log=3, w=10, opts=("gbias_null",)),
    C("thin 32->3 k9 (KW * 4 > 32: not foldable)", 2, 9, 32, 4, 9, reflect=0, cout_log=3),
    C("thin 16->3 k9 reflect", 1, 6, 16, 4, 9, cout_log=3, w=7),
    C("stem 3->64 k7 (thin-fold data gradient), ring mode 1", 1, 64, 4, 64, 7, cin_log=3),
    C("thin data gradient 3->32 k9", 2, 7, 4, 32, 9, cin_log=3, w=9),
    C("discriminator 3->64 k4 s2 (thinin)", 2, 32, 4, 64, 4, s=2, pad=1, cin_log=3, act=LEAKY),
    # ---- Winograd
    C("D-like 64->256 ups2 reflect, N3 (Winograd split<128>, ragged)", 3, 16, 64, 256, 3, ups=2, act=RELU,
      opts=("saved", "pre0", "pre1", "pre2")),
    C("D-like 64->256 ups2 zero, N3", 3, 16, 64, 256, 3, ups=2, reflect=0, opts=("pre0", "pre1", "pre2")),
    C("256->256 zero 20x20, N3 (Winograd DMA GEMM, ragged 256-row tiles)", 3, 20, 256, 256, 3, reflect=0,
      opts=("pre0", "pre1", "pre2")),
    C("256->192 reflect, N3 (Winograd split<64>)", 3, 8, 256, 192, 3, opts=("pre0", "pre1", "pre2")),
    C("R-like 1024->512 (transposed-operand weight gradient), saved", 4, 8, 1024, 512, 3, opts=("saved",)),
    C("R-like 1024->512 (transposed-operand weight gradient), recomputed", 4, 8, 1024, 512, 3, reflect=0),
    C("256->256 ups1 (stream-K Winograd core), recomputed", 2, 8, 256, 256, 3, act=SIGMOID),
    # ---- LDS slab, ring
    C("U4-like 32->64 64x64 (slab with tile statistics, ring 0)", 1, 64, 32, 64, 3, act=RELU),
    C("32->64 66x66 (slab without tile statistics)", 1, 66, 32, 64, 3, reflect=0),
    C("D1-like 32->64 ups2 128x128 (ring 0 at ups 2)", 1, 128, 32, 64, 3, ups=2, act=RELU),
    # ---- direct split-operand and fp32 tiles
    C("1x1 4->1024 32x32, N8 (split<128> with tile statistics)", 8, 32, 4, 1024, 1, cin_log=3),
    C("5x5 16->512 ups2, N8 (split<128> without tile statistics; data gradient split<128,2>)", 8, 30, 16, 512, 5, ups=2),
    C("5x5 128->64 ups2, N8 (data gradient split<128,2>)", 8, 30, 128, 64, 5, ups=2),
    C("1x1 4->64 16x16 (split<64> with tile statistics)", 1, 16, 4, 64, 1, cin_log=3),
    C("1x1 4->64 6x6, N2 (split<64> without tile statistics)", 2, 6, 4, 64, 1, reflect=0, cin_log=3),
    C("32->1024 ups2 odd map, N8 (fp32 <128,128,2,false>)", 8, 30, 32, 1024, 3, ups=2),
    C("128->512 ups2 odd map, N8 (fp32 <128,128>, K > 2048)", 8, 18, 128, 512, 3, ups=2),
    C("64->256 ups2 6x6, N8 (fp32 <128,64>)", 8, 6, 64, 256, 3, ups=2),
    C("1x1 4->128 (fp32 <64,128>)", 1, 3, 4, 128, 1, cin_log=3),
    C("1x1 4->4 (fp32 <64,64>, stream-K <64,64>)", 1, 3, 4, 4, 1, cin_log=3, cout_log=3),
    C("1x1 4->4 6x6, N2 (fp32 <128,32,1>, data gradient split<32,1>)", 2, 6, 4, 4, 1, cin_log=3),
    C("1x1 16->64 ups2 (data gradient split<64,2>)", 2, 12, 16, 64, 1, ups=2),
    C("1x1 16->4 ups2 (data gradient split<64,2,false>)", 2, 12, 16, 4, 1, ups=2),
    # ---- K slices + k_splitk_finish under each epilogue activation
    C("K slices 32->4 k4 s2, act none, cout_log 3", 1, 3, 32, 4, 4, s=2, pad=1, cout_log=3),
    C("K slices 32->4 k4 s2, ReLU", 1, 3, 32, 4, 4, s=2, pad=1, act=RELU),
    C("K slices 32->4 k4 s2, LeakyReLU", 1, 3, 32, 4, 4, s=2, pad=1, act=LEAKY, reflect=0),
    C("K slices 32->4 k4 s2, Tanh", 1, 3, 32, 4, 4, s=2, pad=1, act=TANH),
    C("K slices 32->4 k4 s2, Sigmoid", 1, 3, 32, 4, 4, s=2, pad=1, act=SIGMOID),
    # ---- data gradient: stride 2, K slices, double mirrors
    C("k4 s2 4->4 80x80, N8 (parity classes, plain plan)", 8, 80, 4, 4, 4, s=2, pad=1, cin_log=3),
    C("k4 s2 4->4 4x4 (parity classes, batched re-plan)", 1, 4, 4, 4, 4, s=2, pad=1, cin_log=3),
    C("k4 s2 4->128 4x4 (parity classes, K slices)", 1, 4, 4, 128, 4, s=2, pad=1, cin_log=3),
    C("1x1 4->512 ups2 (data gradient K slices)", 1, 6, 4, 512, 1, ups=2, cin_log=3),
    C("3x3 on a 3-wide map (dbl_mirror)", 1, 3, 4, 4, 3, w=5, cin_log=3),
    C("7x7 pad 3 on a 4x6 map (dbl_mirror)", 1, 4, 4, 4, 7, w=6, cin_log=3),
    C("7x7 pad 3 on a 7x7 map, 16->64 (dbl_mirror)", 2, 7, 16, 64, 7),
    # ---- weight gradient: stream-K tiles, parts, reductions
    C("3x3 4->4 ups2 (stream-K split<64>)", 1, 6, 4, 4, 3, ups=2, cin_log=3),
    C("1x1 32->128 ups2 (stream-K split<128>)", 1, 6, 32, 128, 1, ups=2, cout_log=125),
    C("1x1 4->4 80x80 (> 24 stream-K parts, k_slab_sum)", 1, 80, 4, 4, 1, cin_log=3),
    C("k4 s2 64->1024 (k_wgrad_reduce)", 1, 3, 64, 1024, 4, s=2, pad=1, w=5),
]
CASE_IDS = [c[0] for c in CASES]


def case_desc(case):
    return desc(*case[1])


# ================================================================== the GPU test
def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _reference(x, w, b, dy, g, act, cin_log, cout_log, dtype, device):
    """y = act(conv(pad(unshuffle(x[..., :cin_log]))) + b), dx (physical NHWC, zero on pad channels), dw, db — autograd in `dtype`
    on `device`; b None: no bias, no activation (the |x| * |w| magnitude pass)."""
    xd = x.to(device=device, dtype=dtype).detach().requires_grad_(True)
    wd = w.to(device=device, dtype=dtype).detach().requires_grad_(True)
    xl = xd[..., :cin_log].permute(0, 3, 1, 2)
    if g["ups"] == 2:
        xl = F.pixel_unshuffle(xl, 2)
    p = g["pad"]
    xl = F.pad(xl, (p, p, p, p), mode="reflect" if g["reflect"] else "constant")
    z = F.conv2d(xl, wd, None if b is None else b[:cout_log].to(device=device, dtype=dtype), stride=g["stride"])
    if b is not None:
        z = {NONE: lambda t: t, RELU: torch.relu, LEAKY: lambda t: F.leaky_relu(t, 0.2), TANH: torch.tanh,
             SIGMOID: torch.sigmoid}[act](z)
    dyl = dy[..., :cout_log].permute(0, 3, 1, 2).to(device=device, dtype=dtype)
    # the data / weight gradients of the CONVOLUTION (the entry points take dy after the activation's derivative)
    zlin = F.conv2d(xl, wd, None, stride=g["stride"])
    dx, dw = torch.autograd.grad(zlin, (xd, wd), dyl)
    y = torch.zeros(g["N"], g["Ho"], g["Wo"], g["Cout"], dtype=dtype, device=device)
    y[..., :cout_log] = z.detach().permute(0, 2, 3, 1)
    return y, dx, dw, dyl.sum((0, 2, 3))


def _relmax(got, ref, tol):
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.flatten().argmax())
    return r.flatten()[i].item(), i


def _rel_l2(got, ref):
    d = ref.norm().item()
    return (got.double() - ref).norm().item() / d if d else (got.double() - ref).norm().item()


def _check(what, got, ref64, ref32, A, c, floor, extra=None, l2_floor=1e-7, acc=None):
    """per element |got - ref| <= c U A + floor (+ extra), and the whole tensor within 4x PyTorch-CPU fp32's relative L2
    (+ ||acc|| / ||ref||: the rounding of adding the result into what the buffer held, which PyTorch's result does not carry)"""
    tol = c * U * A + floor + (0 if extra is None else extra)
    worst, i = _relmax(got, ref64, tol)
    assert worst <= 1.0, (f"{what}: element {i} = {got.flatten()[i].item()!r} against float64 {ref64.flatten()[i].item()!r}: "
                          f"{worst:.3g} x its bound (c_path {c:.1f})")
    e, e32 = _rel_l2(got, ref64), _rel_l2(ref32.to(ref64.device), ref64)
    e_acc = 0.0 if acc is None else acc.norm().item() / max(ref64.norm().item(), 1e-300)
    assert e <= max(4 * e32, l2_floor) + e_acc, f"{what}: relative L2 {e:.3e} against float64, PyTorch-CPU fp32 {e32:.3e}"


def _c_path(fp16, kred, partials, wino=False):
    c = (12 + 8 * math.sqrt(kred / 16 + partials)) if fp16 else (2 + 8 * math.sqrt(kred + partials))
    return 16 * c if wino else c


def _l2_floor(fp16):
    """the whole-tensor floor: 1e-7; 2^-22 for the fp16 x 2 kernels, whose operands keep 22 bits — on a short sum (a weight
    gradient over 4 pixels) PyTorch's fp32, exact to 24 bits per product, is far below what 22-bit operands can reach"""
    return 2.0 ** -22 if fp16 else 1e-7


def _profile(lib):
    n = lib.vcg_profile_read(None, 0)
    buf = ctypes.create_string_buffer(max(int(n), 1) + 64)
    lib.vcg_profile_read(buf, len(buf))
    return {ln.split("\t")[0] for ln in buf.value.decode().splitlines() if ln}


FP16_FWD = ("split64", "split128", "slab", "wino", "thinin")
FP16_DGRAD = ("split<128,2>", "split<64,2>", "split<32,1>", "split<64,2,false>", "slab", "wino")


TIERS = (0, 0, 9, 16, 19, 23, 30)


def tier_exponents(n, step=1):
    """-T[i] for i < n, T cycling through TIERS (step 1) or through every third entry of it (step 3: another order of the same
    seven, for the second tensor of a product); index 0 is tier 0 either way, so a dimension of length 1 has tier 0 only and the
    tensor's largest magnitude stays in tier 0"""
    return torch.tensor([-float(TIERS[(step * i) % len(TIERS)]) for i in range(n)], dtype=torch.float64)


def make_operands(case, kind, device="cuda"):
    """(x, wt, bias, dy, g0, gb0) of a case: pad channels zero, as every producer leaves them.
    kind "randn": standard normal draws (the weights at He scale, bias 0.1, the accumulators' prior contents 4).
    kind "tiers": the same draws times exact powers of two, x[n, :, :, c] by 2^-(Tn[n] + Tc[c]), wt[co] by 2^-Tco[co],
    dy[n, :, :, co] by 2^-(Tn'[n] + Tco'[co]) with the tiers of tier_exponents: every output image, output channel, dx image and
    gw[co, ci] is fed by one combination of tiers, most of them 2^-16 ... 2^-60 below the scale the tensor's largest magnitude
    sets; bias, g0 and gb0 as for randn."""
    assert kind in ("randn", "tiers")
    name = case[0]
    g = geom(case_desc(case))
    N, H, W, Cin, Cout, cin_log, cout_log, k = g["N"], g["H"], g["W"], g["Cin"], g["Cout"], g["cin_log"], g["cout_log"], g["KH"]
    seed = sum(map(ord, name)) * 7919
    x = torch.randn((N, H, W, Cin), generator=_gen(seed, device), device=device)
    x[..., cin_log:] = 0
    wt = torch.randn((cout_log, cin_log * g["ups"] ** 2, k, k), generator=_gen(seed + 1, device), device=device)
    wt *= (2.0 / (g["K"])) ** 0.5
    bias = torch.randn((Cout,), generator=_gen(seed + 2, device), device=device) * 0.1
    bias[cout_log:] = 0
    dy = torch.randn((N, g["Ho"], g["Wo"], Cout), generator=_gen(seed + 3, device), device=device)
    dy[..., cout_log:] = 0
    g0 = torch.randn(wt.shape, generator=_gen(seed + 4, device), device=device) * 4.0       # what gw holds before the call
    gb0 = torch.randn((cout_log,), generator=_gen(seed + 5, device), device=device) * 4.0
    if kind == "tiers":
        def p2(e):
            return torch.exp2(e).to(device=device, dtype=torch.float32)
        x *= p2(tier_exponents(N)[:, None, None, None] + tier_exponents(Cin)[None, None, None, :])
        wt *= p2(tier_exponents(cout_log)[:, None, None, None])
        dy *= p2(tier_exponents(N, 3)[:, None, None, None] + tier_exponents(Cout, 3)[None, None, None, :])
    return x, wt, bias, dy, g0, gb0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_conv_plan_against_float64(case, pkg, device):
    run_conv_plan(case, pkg, device, "randn")


def run_conv_plan(case, pkg, device, kind):
    """Everything the module docstring lists, on the operands make_operands(case, kind) builds.  kind "tiers" leaves the
    vcg_conv_fwd_in_pre options out: that operand is normalised by construction."""
    name, _, opts = case
    if kind != "randn":
        name = f"{name} [{kind}]"
        opts = tuple(o for o in opts if not o.startswith("pre"))
    lib, nat = pkg._native.lib(), pkg._native
    cd = case_desc(case)
    plan = conv_plan(cd)
    g, pf, pd, pw = plan["g"], plan["fwd"], plan["dgrad"], plan["wgrad"]
    N, H, W, Cin, Cout, cin_log, cout_log, act = g["N"], g["H"], g["W"], g["Cin"], g["Cout"], g["cin_log"], g["cout_log"], g["act"]
    Ho, Wo, k = g["Ho"], g["Wo"], g["KH"]
    seed = sum(map(ord, case[0])) * 7919
    st = _st()
    x, wt, bias, dy, g0, gb0 = make_operands(case, kind, device)

    def pack(flags):
        cdp = case_desc(case)
        cdp[14] = flags
        buf = Out((lib.vcg_pack_weight_floats(cdp),), device)
        nat.check(lib.vcg_pack_weight(P(wt), P(buf.t), cdp, st), "vcg_pack_weight")
        return buf.t

    wf = pack(0)
    reads_wf = lib.vcg_conv_reads_wf(cd)
    assert reads_wf == reads_wf_mirror(cd)

    def fwd(wfp):
        y = Out((N, Ho, Wo, Cout), device)
        ws = _ws(lib.vcg_conv_fwd_workspace(cd), device)
        nat.check(lib.vcg_conv_fwd(P(x), P(wfp), P(bias), P(y.t), cd, P(ws), ws.numel() * 4, st), "vcg_conv_fwd")
        return y.check("vcg_conv_fwd")

    def fwd_in(wfp, saved=None, xin=x, pre=None):
        y, mean, rstd = Out((N, Ho, Wo, Cout), device), Out((N, Cout), device), Out((N, Cout), device)
        ws = _ws(lib.vcg_conv_fwd_in_workspace(cd), device)
        if pre is None:
            nat.check(lib.vcg_conv_fwd_in(P(xin), P(wfp), P(bias), P(y.t), P(mean.t), P(rstd.t), EPS, P(saved), cd, P(ws),
                                          ws.numel() * 4, st), "vcg_conv_fwd_in")
        else:
            pm, pr, pa = pre
            nat.check(lib.vcg_conv_fwd_in_pre(P(xin), P(pm), P(pr), pa, P(wfp), P(bias), P(y.t), P(mean.t), P(rstd.t), EPS,
                                              P(saved), cd, P(ws), ws.numel() * 4, st), "vcg_conv_fwd_in_pre")
        return y.check("vcg_conv_fwd_in"), mean.check("mean"), rstd.check("rstd")

    def dgrad(wfp):
        dx = Out((N, H, W, Cin), device)
        ws = _ws(lib.vcg_conv_dgrad_workspace(cd), device)
        nat.check(lib.vcg_conv_dgrad(P(dy), P(wfp), P(dx.t), cd, P(ws), ws.numel() * 4, st), "vcg_conv_dgrad")
        return dx.check("vcg_conv_dgrad")

    def wgrad(xin=x, saved=None):
        gw = Out(tuple(wt.shape), device, fill=g0)
        gb = None if "gbias_null" in opts else Out((cout_log,), device, fill=gb0)
        ws = _ws(lib.vcg_conv_wgrad_workspace(cd), device)
        nat.check(lib.vcg_conv_wgrad_saved(P(xin), P(dy), P(gw.t), None if gb is None else P(gb.t), P(saved), cd, P(ws),
                                           ws.numel() * 4, st), "vcg_conv_wgrad")
        return gw.check("gw"), None if gb is None else gb.check("gbias")

    def twice(fn, *a, **kw):
        """run twice on fresh NaN buffers: the results must be bitwise equal (deterministic reductions)"""
        r1, r2 = fn(*a, **kw), fn(*a, **kw)
        torch.cuda.synchronize()
        for u, v in zip(r1 if isinstance(r1, tuple) else (r1,), r2 if isinstance(r2, tuple) else (r2,)):
            if u is not None:
                assert torch.equal(u.view(torch.int32), v.view(torch.int32)), f"{name}: {fn.__name__} is not deterministic"
        return r1

    has_dgrad = pd["branch"] != "unsupported"
    nsaved = lib.vcg_conv_saved_floats(cd)
    _profile(lib)
    lib.vcg_profile_enable(1)
    try:
        y = twice(fwd, wf)
        yi, mean, rstd = twice(fwd_in, wf)
        dx = twice(dgrad, wf) if has_dgrad else None
        gw, gb = twice(wgrad)
        saved = None
        if "saved" in opts:
            assert nsaved > 0, f"{name}: no forward state to keep at this geometry"
            saved = _ws(nsaved * 4, device)
            fwd_in(wf, saved=saved)
            gws, gbs = twice(wgrad, saved=saved)
        torch.cuda.synchronize()
        seen = _profile(lib)
    finally:
        lib.vcg_profile_enable(0)
    # ---- branch witness
    for what, p in (("forward", pf), ("data gradient", pd), ("weight gradient", pw)):
        if p.get("kernel") and (what != "data gradient" or has_dgrad):
            assert p["kernel"] in seen, f"{name}: the {what} should run {p['kernel']} ({p['branch']}); the profile saw {sorted(seen)}"

    # ---- references: float64 on the device, fp32 on the CPU, magnitudes |x| * |w|
    y64, dx64, dw64, db64 = _reference(x, wt, bias, dy, g, act, cin_log, cout_log, torch.float64, device)
    y32, dx32, dw32, db32 = _reference(x.cpu(), wt.cpu(), bias.cpu(), dy.cpu(), g, act, cin_log, cout_log, torch.float32, "cpu")
    Ay, Adx, Adw, Adb = _reference(x.abs(), wt.abs(), None, dy.abs(), g, NONE, cin_log, cout_log, torch.float64, device)
    ax, aw, ady = x.abs().max().item(), wt.abs().max().item(), dy.abs().max().item()
    wino_f = pf["branch"] == "wino"
    kf = g["kc"] * 9 if wino_f else g["K"]
    fp16_f = pf["branch"] in FP16_FWD or (pf["branch"] == "thin_fold" and bool(pf["kernel"]))
    c_f = _c_path(fp16_f, kf, pf["nsplit"] + k, wino_f)
    fl_f = 2.0 ** -40 * 2 * kf * ax * aw * (16 if wino_f else 1)
    for what, got in (("forward", y), ("forward with statistics", yi)):
        assert (got[..., cout_log:] == 0).all(), f"{name}: {what} wrote a nonzero pad channel"
        _check(f"{name}: {what}", got, y64, y32, Ay, c_f, fl_f, extra=4 * U * y64.abs(), l2_floor=_l2_floor(fp16_f))
    ym = yi.double().reshape(N, Ho * Wo, Cout)
    m64, v64 = ym.mean(1), ym.var(1, unbiased=False)
    r64 = 1.0 / torch.sqrt(v64 + EPS)
    assert ((mean.double() - m64).abs() / (v64.sqrt() + m64.abs() + 1e-6)).max().item() <= 1e-6, f"{name}: mean"
    assert ((rstd.double() - r64).abs() / r64).max().item() <= 3e-6, f"{name}: rstd"
    if has_dgrad:
        wino_d = pd["branch"] == "wino"
        kd = k * k * Cout
        fp16_d = pd["branch"] in FP16_DGRAD or (pd["branch"] == "thin_fold" and bool(pd["kernel"]))
        c_d = _c_path(fp16_d, kd, pd["nsplit"] + 9, wino_d)
        assert (dx[..., cin_log:] == 0).all(), f"{name}: the data gradient wrote a nonzero pad channel"
        _check(f"{name}: data gradient", dx, dx64, dx32, Adx, c_d, 2.0 ** -40 * 2 * 4 * kd * ady * aw * (16 if wino_d else 1),
               l2_floor=_l2_floor(fp16_d))
    wino_w = pw["branch"].startswith("wino")
    kw_ = wino_T(g) * 16 if wino_w else g["M"]
    fp16_w = wino_w or pw["branch"].startswith("ring") or pw["kernel"] != "k_conv_wgrad<fp32 MFMA>"
    c_w = _c_path(fp16_w, kw_, pw["parts"] + 16, wino_w)
    fl_w = 2.0 ** -40 * 2 * kw_ * ax * ady * (16 if wino_w else 1)
    results = [("weight gradient", gw, gb)] + ([("weight gradient from saved", gws, gbs)] if saved is not None else [])
    for what, gwt, gbt in results:
        _check(f"{name}: {what}", gwt.double() - g0.double(), dw64, dw32, Adw, c_w, fl_w, extra=U * (g0.abs() + dw64.abs()),
               l2_floor=_l2_floor(fp16_w), acc=U * (g0.abs() + dw64.abs()))
        if gbt is not None:
            _check(f"{name}: {what} (bias)", gbt.double() - gb0.double(), db64, db32, Adb, _c_path(False, g["M"], 16), 0,
                   extra=U * (gb0.abs() + db64.abs()), l2_floor=_l2_floor(True), acc=U * (gb0.abs() + db64.abs()))

    # ---- the Wf claim: a pack without the fp32 Wf block gives bitwise the same forward, statistics and data gradient
    if reads_wf == 0:
        wf2 = pack(1)
        assert torch.equal(fwd(wf2).view(torch.int32), y.view(torch.int32)), f"{name}: forward differs without Wf"
        y2, m2, r2 = fwd_in(wf2)
        assert torch.equal(y2.view(torch.int32), yi.view(torch.int32)) and torch.equal(m2, mean) and torch.equal(r2, rstd), \
            f"{name}: forward with statistics differs without Wf"
        if has_dgrad:
            assert torch.equal(dgrad(wf2).view(torch.int32), dx.view(torch.int32)), f"{name}: data gradient differs without Wf"

    # ---- vcg_conv_fwd_in_pre: the normalising gather against pre_act((t_prev - mean) rstd) in float64
    for pa in opts_pre(opts):
        assert pf["pre_ok"] and lib.vcg_conv_pre_ok(cd) == 1
        spread = torch.exp(torch.randn((N, 1, 1, Cin), generator=_gen(seed + 6 + pa, device), device=device) * 0.5)
        off = torch.randn((N, 1, 1, Cin), generator=_gen(seed + 9 + pa, device), device=device) * 3.0 * spread
        t_prev = x * spread + off
        t_prev[..., cin_log:] = 0
        tv = t_prev.double().reshape(N, H * W, Cin)
        pm = tv.mean(1).float()
        pr = (1.0 / torch.sqrt(tv.var(1, unbiased=False) + EPS)).float()
        xn = (t_prev.double() - pm.double()[:, None, None, :]) * pr.double()[:, None, None, :]
        xn = {NONE: lambda t: t, RELU: torch.relu, LEAKY: lambda t: F.leaky_relu(t, 0.2)}[pa](xn)
        xn[..., cin_log:] = 0
        sv = _ws(nsaved * 4, device) if nsaved else None
        yp, mp, rp = fwd_in(wf, saved=sv, xin=t_prev, pre=(pm, pr, pa))
        yp64, _, dwp64, _ = _reference(xn, wt, bias, dy, g, act, cin_log, cout_log, torch.float64, device)
        yp32, _, dwp32, _ = _reference(xn.float().cpu(), wt.cpu(), bias.cpu(), dy.cpu(), g, act, cin_log, cout_log, torch.float32, "cpu")
        Ayp, _, Adwp, _ = _reference(xn.abs(), wt.abs(), None, dy.abs(), g, NONE, cin_log, cout_log, torch.float64, device)
        bound = math.sqrt(H * W)                    # the gather's operand scale: |xhat| <= sqrt(HW), not measured
        # + the rounding of the normalised input itself (t - mean) * rstd in fp32: U (|t| + |mean|) rstd per element
        xerr = (t_prev.abs().double() + pm.abs().double()[:, None, None, :]) * pr.double()[:, None, None, :] * 2 * U
        xerr[..., cin_log:] = 0
        Aerr, _, _, _ = _reference(xerr, wt.abs(), None, dy.abs(), g, NONE, cin_log, cout_log, torch.float64, device)
        assert (yp[..., cout_log:] == 0).all(), f"{name}: pre act{pa}: nonzero pad channel"
        _check(f"{name}: fwd_in_pre act{pa}", yp, yp64, yp32, Ayp, c_f, 2.0 ** -40 * 2 * kf * bound * aw * 16,
               extra=4 * U * yp64.abs() + Aerr, l2_floor=_l2_floor(True))
        ypm = yp.double().reshape(N, Ho * Wo, Cout)
        m64p, v64p = ypm.mean(1), ypm.var(1, unbiased=False)
        assert ((mp.double() - m64p).abs() / (v64p.sqrt() + m64p.abs() + 1e-6)).max().item() <= 1e-6, f"{name}: pre act{pa} mean"
        assert ((rp.double() - 1.0 / torch.sqrt(v64p + EPS)).abs() * torch.sqrt(v64p + EPS)).max().item() <= 3e-6, \
            f"{name}: pre act{pa} rstd"
        if sv is not None:
            gwp, _ = wgrad(xin=t_prev, saved=sv)
            _check(f"{name}: weight gradient from the pre-gather's saved state act{pa}", gwp.double() - g0.double(), dwp64, dwp32,
                   Adwp, c_w, 2.0 ** -40 * 2 * kw_ * bound * ady * 16, extra=U * (g0.abs() + dwp64.abs()), l2_floor=_l2_floor(True),
                   acc=U * (g0.abs() + dwp64.abs()))


def reads_wf_mirror(cd):
    return reads_wf(geom(cd))
