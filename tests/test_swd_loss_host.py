"""CPU: the sliced Wasserstein training loss (csrc/swd_loss.hip, ops.swd_loss, Losses.SlicedWassersteinLoss) — what needs no GPU:
the C ABI and its refusals, the cell-side rule, the flags and configure_loss, the plan sequence of the loss object — and the
float64 restatement of the definition ("Sliced Wasserstein training loss") that tests/test_gpu_swd_loss.py holds the
device against."""
import ctypes
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vcg_swd_loss_levels", "vcg_swd_cell_side", "vcg_swd_pool", "vcg_swd_pool_adjoint_add", "vcg_swd_grid_gather",
           "vcg_swd_grid_scatter", "vcg_sort_columns_indexed", "vcg_swd_pair_loss_workspace", "vcg_swd_pair_loss",
           "vcg_swd_unit_columns")
PATCH, CAP, MIN_CELL, MIN_SIDE = 7, 8192, 8, 16


# ------------------------------------------------------------------ the definition, restated
def levels_of(h, w, cap=3):
    n = 1
    while n < cap and h % 2 == 0 and w % 2 == 0 and h // 2 >= MIN_SIDE and w // 2 >= MIN_SIDE:
        h, w, n = h // 2, w // 2, n + 1
    return n


def cell_side(n_images, h, w):
    s = MIN_CELL
    while n_images * (h // s) * (w // s) > CAP:
        s += 1
    return s


def pool_ref(x):
    """(N, 3, H, W) -> the 2 x 2 mean (torch or numpy, any dtype)."""
    return (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) * 0.25


def grid_gather_ref(level, s, oy, ox):
    """(N, 3, H, W) -> (N cy cx, 147): the patch at (oy, ox) of every s x s cell, flattened (c, dy, dx)."""
    if not isinstance(level, torch.Tensor):
        return grid_gather_ref(torch.from_numpy(np.ascontiguousarray(level)), s, oy, ox).numpy()
    n, _, h, w = level.shape
    cy, cx = h // s, w // s
    cells = level[:, :, :cy * s, :cx * s].reshape(n, 3, cy, s, cx, s)[:, :, :, oy:oy + PATCH, :, ox:ox + PATCH]
    return cells.permute(0, 2, 4, 1, 3, 5).reshape(n * cy * cx, 3 * PATCH * PATCH)      # (image, cell row, cell column) x (c, dy, dx)


def grid_gather_loop(level, s, oy, ox):
    """The same, one slice per cell: what the vectorised form is checked against."""
    n, _, h, w = level.shape
    return np.stack([level[i, :, a * s + oy:a * s + oy + PATCH, b * s + ox:b * s + ox + PATCH].reshape(-1)
                     for i in range(n) for a in range(h // s) for b in range(w // s)])


def swd_loss_ref(a, b, levels, offsets, dirs, dtype=torch.float64):
    """The loss of torch CPU tensors in `dtype`, differentiable in a: a stable sort per direction, the mean over (d, i) per level,
    the mean over the levels."""
    a, b, dirs = a.to(dtype), b.to(dtype), dirs.to(dtype)
    total = 0.0
    for k in range(levels):
        if k:
            a, b = pool_ref(a), pool_ref(b)
        s = cell_side(a.shape[0], a.shape[2], a.shape[3])
        oy, ox = offsets[k]
        pa = grid_gather_ref(a, s, oy, ox) @ dirs
        pb = grid_gather_ref(b, s, oy, ox) @ dirs
        sa = torch.sort(pa, dim=0, stable=True).values
        sb = torch.sort(pb, dim=0, stable=True).values
        total = total + (sa - sb).abs().mean()
    return total / levels


# ------------------------------------------------------------------ the C ABI
def test_header_exports_and_binding_have_the_entries(pkg):
    text = open(os.path.join(ROOT, "include", "vcg.h")).read()
    assert int(re.search(r"#define\s+VCG_SWD_LOSS_MAX_DESC\s+(\d+)", text).group(1)) == CAP
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vcg_[a-z0-9_]+)\s*\(", text))
    path = pkg._native.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/vcg.h"
        assert name in exported, f"{name} is not exported by libvcg.so"
        assert name in pkg._native.SIGNATURES, f"{name} is not in the ctypes table"
    assert "swd_loss.hip" in pkg._native.SOURCES
    assert pkg._native.lib().vcg_abi_version() == 6            # the entries are additive


def test_cell_side_and_level_count(pkg):
    ops, lib = pkg.ops, pkg._native.lib()
    for (n, h, w), (s, count) in {(8, 256, 256): (8, 8192), (9, 256, 256): (9, 7056), (2, 16, 16): (8, 8),
                                  (16, 256, 256): (12, 7056), (3, 40, 24): (8, 45), (1, 64, 64): (8, 64)}.items():
        assert ops.swd_cell_side(n, h, w) == s == cell_side(n, h, w)
        assert n * (h // s) * (w // s) == count
    for n, h, w in [(1, 16, 16), (5, 100, 36), (64, 128, 128), (33, 250, 130), (8192, 16, 16), (2048, 32, 32)]:
        assert ops.swd_cell_side(n, h, w) == cell_side(n, h, w)
    for bad in [(0, 16, 16), (1, 15, 16), (1, 16, 15), (1, 40000, 16)]:
        assert lib.vcg_swd_cell_side(*bad) == 0 and b"vcg_swd_cell_side" in lib.vcg_last_error()
        with pytest.raises(RuntimeError, match="vcg_swd_cell_side"):
            ops.swd_cell_side(*bad)
    assert lib.vcg_swd_cell_side(8193, 16, 16) == 0 and b"8192" in lib.vcg_last_error()     # one cell per image is already too many
    for (h, w), want in {(16, 16): 1, (40, 24): 1, (32, 32): 2, (64, 64): 3, (256, 256): 3, (64, 36): 2, (62, 64): 2, (30, 64): 1, (33, 64): 1,
                      (128, 32): 2}.items():
        assert ops.swd_loss_levels(h, w) == want == levels_of(h, w)
    assert lib.vcg_swd_loss_levels(15, 64) == 0 and b"vcg_swd_loss_levels" in lib.vcg_last_error()
    assert [g[:3] for g in ops.swd_loss_geometry(1, 64, 64, 3)] == [(64, 64, 8), (32, 32, 8), (16, 16, 8)]
    for bad in (0, 4, True, 1.5):
        with pytest.raises(RuntimeError, match="levels"):
            ops.swd_loss_geometry(1, 64, 64, bad)
    with pytest.raises(RuntimeError, match="3 levels asked of 32x32 images, which have 2"):
        ops.swd_loss_geometry(1, 32, 32, 3)
    with pytest.raises(RuntimeError, match="have 1"):              # a side under 16 for the requested level
        ops.swd_loss_geometry(3, 40, 24, 2)


def test_bad_arguments_are_rejected_without_touching_the_gpu(pkg):
    lib = pkg._native.lib()
    buf = (ctypes.c_double * 256)()                             # host memory: only ever inspected as an address
    base = ctypes.addressof(buf)
    base += -base % 16
    P = ctypes.c_void_p
    p = [P(base + 64 * i) for i in range(8)]

    def err():
        return lib.vcg_last_error().decode()

    # pool and its adjoint
    for fn in (lib.vcg_swd_pool, lib.vcg_swd_pool_adjoint_add):
        assert fn(None, p[1], 1, 32, 32, None) != 0 and "null pointer" in err()
        assert fn(p[0], None, 1, 32, 32, None) != 0 and "null pointer" in err()
        assert fn(p[0], p[1], 0, 32, 32, None) != 0 and "N=0" in err()
        assert fn(p[0], p[1], 1, 16, 32, None) != 0 and "no coarser" in err()      # the half would be 8
        assert fn(p[0], p[1], 1, 34, 33, None) != 0 and "no coarser" in err()      # odd
        assert fn(p[0], p[0], 1, 32, 32, None) != 0 and "distinct" in err()
        assert fn(P(base + 4), p[1], 1, 32, 32, None) != 0 and "aligned" in err()

    # grid gather / scatter: N, H, W, s, oy, ox
    def gather(level=p[0], out=p[1], g=(2, 32, 32, 8, 0, 0)):
        return lib.vcg_swd_grid_gather(level, out, *g, None)

    def scatter(gdesc=p[0], gscale=None, scale=1.0, out=p[1], g=(2, 32, 32, 8, 0, 0)):
        return lib.vcg_swd_grid_scatter(gdesc, gscale, scale, out, *g, None)

    for call in (gather, scatter):
        assert call(g=(0, 32, 32, 8, 0, 0)) != 0 and "N=0" in err()
        assert call(g=(2, 15, 32, 8, 0, 0)) != 0 and "15x32" in err()
        assert call(g=(2, 32, 32, 7, 0, 0)) != 0 and "cell side 7" in err()
        assert call(g=(2, 32, 32, 33, 0, 0)) != 0 and "cell side 33" in err()
        assert call(g=(2, 32, 32, 8, 2, 0)) != 0 and "offset (2, 0) outside [0, 1]" in err()
        assert call(g=(2, 32, 32, 8, 0, -1)) != 0 and "offset (0, -1)" in err()
        assert call(g=(2, 32, 32, 9, 0, 3)) != 0 and "offset (0, 3) outside [0, 2]" in err()
        assert call(g=(9, 256, 256, 8, 0, 0)) != 0 and "9216 descriptors (1 .. 8192)" in err()
    assert gather(level=None) != 0 and "null pointer" in err()
    assert gather(out=None) != 0 and "null pointer" in err()
    assert scatter(gdesc=None) != 0 and "null pointer" in err()
    assert scatter(out=None) != 0 and "null pointer" in err()
    assert scatter(scale=float("nan")) != 0 and "finite" in err()
    assert scatter(out=P(base + 72)) != 0 and "aligned" in err()

    # indexed sort: x, keys, rows, n, cols, row stride, column stride
    def sort(x=p[0], keys=p[1], rows=p[2], n=8, cols=2, rs=1, cs=8):
        return lib.vcg_sort_columns_indexed(x, keys, rows, n, cols, rs, cs, None)

    assert sort(n=0) != 0 and "0 rows (1 .. 8192" in err()
    assert sort(n=8193, cs=8193) != 0 and "8193 rows (1 .. 8192" in err()
    assert sort(cols=0) != 0 and "cols=0" in err()
    assert sort(rs=1, cs=7) != 0 and "dense" in err()
    assert sort(keys=p[2]) != 0 and "distinct" in err()
    for name in ("x", "keys", "rows"):
        assert sort(**{name: None}) != 0 and "null pointer" in err()

    # pair loss
    assert lib.vcg_swd_pair_loss_workspace(0, 128) == 0 and "0 descriptors" in err()
    assert lib.vcg_swd_pair_loss_workspace(8193, 128) == 0 and "8193 descriptors (1 .. 8192)" in err()
    assert lib.vcg_swd_pair_loss_workspace(64, 0) == 0 and "0 directions" in err()
    assert lib.vcg_swd_pair_loss_workspace(64, 1025) == 0 and "1025 directions" in err()
    need = lib.vcg_swd_pair_loss_workspace(8192, 128)
    assert need >= 8192 * 128 // 2048 * 8 and need % 16 == 0

    def pair(a=p[0], b=p[1], perm=p[2], gproj=p[3], n=64, ndir=128, weight=1.0, acc=0, total=p[4], out=p[5], ws=p[6], need=1 << 20):
        return lib.vcg_swd_pair_loss(a, b, perm, gproj, n, ndir, weight, acc, total, out, ws, need, None)

    for name in ("a", "b", "perm", "gproj", "total", "out", "ws"):
        assert pair(**{name: None}) != 0 and "null pointer" in err()
    assert pair(n=0) != 0 and "0 descriptors" in err()
    assert pair(n=8193) != 0 and "8193 descriptors" in err()
    assert pair(ndir=0) != 0 and "directions" in err()
    assert pair(weight=float("inf")) != 0 and "finite" in err()
    assert pair(need=8) != 0 and "workspace of 8 bytes" in err()
    assert pair(gproj=p[0]) != 0 and "alias" in err()
    assert pair(ws=P(base + 64 * 6 + 8)) != 0 and "aligned" in err()

    # unit columns
    assert lib.vcg_swd_unit_columns(None, p[1], 147, 128, None) != 0 and "null pointer" in err()
    assert lib.vcg_swd_unit_columns(p[0], None, 147, 128, None) != 0 and "null pointer" in err()
    assert lib.vcg_swd_unit_columns(p[0], p[1], 0, 128, None) != 0 and "K=0" in err()
    assert lib.vcg_swd_unit_columns(p[0], p[1], 147, 0, None) != 0 and "D=0" in err()


def test_ops_refuse_before_the_library_is_asked(pkg):
    ops = pkg.ops
    img = torch.zeros(1, 3, 32, 32)
    plan = ops.SwdPlan(((0, 0),), torch.zeros(147, 128))
    with pytest.raises(RuntimeError, match="cuda"):
        ops.swd_loss(img, img, 1, plan)
    with pytest.raises(RuntimeError, match="must not require a gradient"):
        ops.swd_loss(img, img.clone().requires_grad_(True), 1, plan)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.swd_loss(img, torch.zeros(1, 3, 32, 16), 1, plan)
    with pytest.raises(RuntimeError, match=r"\(N, 3, H, W\)"):
        ops.swd_loss(torch.zeros(1, 4, 32, 32), torch.zeros(1, 4, 32, 32), 1, plan)
    for fn, args in ((ops.swd_pool, (img,)), (ops.swd_grid_gather, (img, 8, 0, 0)), (ops.sort_columns_indexed, (torch.zeros(4, 2),)),
                     (ops.swd_unit_columns, (torch.zeros(4, 2),)), (ops.swd_grid_scatter, (torch.zeros(16, 147), (1, 32, 32), 8, 0, 0))):
        with pytest.raises(RuntimeError, match="cuda"):
            fn(*args)


# ------------------------------------------------------------------ flags, configure_loss
@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module("vae-cyclegan-implementation_amd.train")


def test_flags_parse_and_reach_configure_loss(pkg, train, capsys):
    p = train.build_parser()
    args = p.parse_args([])
    assert args.lambda_swd == 0.0 and args.swd_levels == 3
    args = p.parse_args(["--architecture", "cyclevae", "--unpaired", "--lambda_swd", "0.25", "--swd_levels", "2"])
    assert args.lambda_swd == 0.25 and args.swd_levels == 2
    saved = json.loads(json.dumps(vars(args)))                  # what args.json holds
    assert saved["lambda_swd"] == 0.25 and saved["swd_levels"] == 2
    for flag, bad in (("--lambda_swd", "-1"), ("--lambda_swd", "nan"), ("--lambda_swd", "inf"), ("--lambda_swd", "x"),
                      ("--swd_levels", "0"), ("--swd_levels", "4")):
        with pytest.raises(SystemExit):
            p.parse_args([flag, bad])
        assert flag in capsys.readouterr().err
    N = pkg.Networks
    for make in (lambda: N.CycleAE(paired=False), lambda: N.CycleVAE(latent_dim=8, paired=True),
                 lambda: N.CycleAEGAN(paired=False), lambda: N.CycleVAEGAN(latent_dim=8, paired=True)):
        m = make()
        assert m.swd_term is None and not m.swd_enabled
        m.configure_loss()
        assert m.swd_term is None
        m.configure_loss(lambda_swd=0.0, swd_levels=7)          # weight 0: no loss object, the option is not looked at
        assert m.swd_term is None and "loss_swd" not in dict(m._report_spec(True))
        m.configure_loss(lambda_swd=args.lambda_swd, swd_levels=args.swd_levels, swd_seed=5)
        lam, fn = m.swd_term
        assert lam == 0.25 and isinstance(fn, pkg.Losses.SlicedWassersteinLoss) and (fn.levels, fn.seed, fn.step) == (2, 5, 0)
        assert m.swd_enabled and not any(isinstance(c, pkg.Losses.SlicedWassersteinLoss) for c in m.modules())     # no new state_dict key
        for training in (True, False):
            names = [n for n, _ in m._report_spec(training) if n not in ("Gx", "Fy")]
            assert names[-1] == "loss_swd"
        assert m.save_swd_state() == fn.state_dict()
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="lambda_swd"):
                m.configure_loss(lambda_swd=bad)
        with pytest.raises(ValueError, match="levels"):
            m.configure_loss(lambda_swd=1.0, swd_levels=4)


def test_a_positive_weight_is_refused_by_the_single_direction_models(pkg, train):
    N = pkg.Networks
    for make in (N.Autoencoder, lambda: N.VariationalAutoencoder(latent_dim=8), N.DoubleAutoencoder,
                 lambda: N.DoubleVariationalAutoencoder(latent_dim=8), N.AEGAN, lambda: N.VAEGAN(latent_dim=8)):
        m = make()
        m.configure_loss(lambda_swd=0.0)                        # one call fits every architecture
        with pytest.raises(ValueError, match="lambda_swd") as e:
            m.configure_loss(lambda_swd=0.5)
        for name in ("cycleae", "cyclevae", "cycleaegan", "cyclevaegan"):
            assert name in str(e.value)
        with pytest.raises(ValueError, match="lambda_swd"):
            m.configure_loss(lambda_swd=-0.5)
        with pytest.raises(RuntimeError, match="no sliced Wasserstein term"):
            N.CycleAE().save_swd_state()
    for arch in ("autoencoder", "vae", "doubleae", "doublevae", "aegan", "vaegan"):
        args = train.build_parser().parse_args(["--architecture", arch, "--lambda_swd", "0.5"])
        with pytest.raises(ValueError, match="lambda_swd") as e:
            train.main(args)                                    # before any device is touched
        assert "the flag would be ignored" in str(e.value) and all(n in str(e.value) for n in train.SWD_ARCHS)
    args = train.build_parser().parse_args(["--architecture", "cyclevae"])
    for bad in (-1.0, float("nan")):
        args.lambda_swd = bad
        with pytest.raises(ValueError, match="lambda_swd"):
            train.main(args)
    args.lambda_swd, args.swd_levels = 1.0, 5
    with pytest.raises(ValueError, match="swd_levels"):
        train.main(args)


# ------------------------------------------------------------------ the loss object
def test_offsets_depend_on_seed_and_step_and_survive_a_state_dict_round_trip(pkg):
    L = pkg.Losses.SlicedWassersteinLoss
    for bad in (0, 4, 2.5, True):
        with pytest.raises(ValueError, match="levels"):
            L(levels=bad)
    with pytest.raises(ValueError, match="seed"):
        L(seed=-1)
    a, b, c = L(levels=3, seed=11), L(levels=3, seed=11), L(levels=3, seed=12)
    shape = (9, 256, 256)                                       # cells of 9, 8, 8: offsets in [0, 2], [0, 1], [0, 1]
    seq_a = [a.offsets(*shape, step=t) for t in range(40)]
    assert seq_a == [b.offsets(*shape, step=t) for t in range(40)]
    assert seq_a != [c.offsets(*shape, step=t) for t in range(40)]
    assert len(set(seq_a)) > 10                                 # fresh offsets from step to step
    for offs in seq_a:
        assert len(offs) == 3
        for (oy, ox), hi in zip(offs, (2, 1, 1)):
            assert 0 <= oy <= hi and 0 <= ox <= hi
    assert {o[0][0] for o in seq_a} == {0, 1, 2}                # both ends of the range are reached
    assert a.offsets(*shape) == seq_a[0]                        # the next call's, without advancing
    a.step = 17
    state = a.state_dict()
    assert state["_extra_state"] == {"seed": 11, "step": 17, "levels": 3}
    d = L(levels=3, seed=99)
    d.load_state_dict(json.loads(json.dumps(state)))            # plain data: a checkpoint holds it as is
    assert (d.seed, d.step) == (11, 17) and d.offsets(*shape) == seq_a[17]
    with pytest.raises(ValueError, match="levels"):
        L(levels=2).load_state_dict(state)
    assert L.DIRECTION_QUADS * 4 >= 147 * 128                   # consecutive steps draw disjoint Gaussians


def test_restatement_is_zero_on_equal_sets_sees_a_colour_shift_and_needs_no_pairing():
    rng = np.random.RandomState(0)
    odd = rng.rand(3, 3, 40, 29)
    for s, oy, ox in ((8, 0, 1), (9, 2, 0), (13, 6, 3)):
        assert np.array_equal(grid_gather_ref(odd, s, oy, ox), grid_gather_loop(odd, s, oy, ox))
    a = torch.from_numpy(rng.rand(4, 3, 32, 32))
    dirs = torch.from_numpy(rng.randn(147, 128))
    dirs = dirs / dirs.norm(dim=0, keepdim=True)
    offs = ((1, 0), (0, 1))
    assert float(swd_loss_ref(a, a.clone(), 2, offs, dirs)) == 0.0
    perm = torch.tensor([2, 0, 3, 1])
    assert float(swd_loss_ref(a, a[perm], 2, offs, dirs)) < 1e-15          # the same SET of images: no pairing is looked at
    shifted = a + torch.tensor([0.1, 0.0, 0.0]).reshape(1, 3, 1, 1)
    assert float(swd_loss_ref(shifted, a, 2, offs, dirs)) > 1e-3           # the descriptors are not normalised
    x = a.clone().requires_grad_(True)
    swd_loss_ref(x, torch.from_numpy(rng.rand(4, 3, 32, 32)), 2, offs, dirs).backward()
    g = x.grad
    inside = torch.zeros(32, 32, dtype=torch.bool)
    for cy in range(4):
        for cx in range(4):
            inside[cy * 8 + 1:cy * 8 + 8, cx * 8:cx * 8 + 7] = True
    assert (g[..., 7::8] != 0).any()                                       # level 1 reaches pixels level 0's patches skip
    lvl0_only = x.detach().clone().requires_grad_(True)
    swd_loss_ref(lvl0_only, a[perm] * 0.5, 1, offs[:1], dirs).backward()
    assert (lvl0_only.grad[..., ~inside] == 0).all() and (lvl0_only.grad[..., inside] != 0).any()
