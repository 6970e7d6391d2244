"""GPU: the sliced Wasserstein training loss (csrc/swd_loss.hip, ops.swd_loss, Losses.SlicedWassersteinLoss) stage by stage
against numpy / float64, its bitwise properties, its gradient against the float64 restatement of tests/test_swd_loss_host.py, and
the term inside the cycle models' steps.  VCG_SWD_LOSS_ERROR_LOG=<file> writes the observed errors (profiles/swd_loss_error.txt).

The cycleaegan step runs at 256 x 256: its discriminators' last layer spans the whole 16 x 16 map of a 256 x 256 input, the one
size they take; cyclevae, which has none, runs at 64 x 64."""
import os

import numpy as np
import pytest
import torch

import test_swd_loss_host as ref
from test_gpu_swd import _sort_input

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ERRORS = []
# the shapes the end-to-end checks run: (N, H, W), levels
E2E = [((2, 16, 16), 1), ((3, 40, 24), 1), ((1, 64, 64), 3), ((9, 256, 256), 1)]


@pytest.fixture(scope="module", autouse=True)
def _error_log():
    yield
    path = os.environ.get("VCG_SWD_LOSS_ERROR_LOG")
    if path and ERRORS:
        with open(path, "w") as f:
            f.write("# sliced Wasserstein training loss: observed error of the device kernels against the float64 restatement\n")
            f.write("\n".join(ERRORS) + "\n")


def _note(line):
    ERRORS.append(line)
    print(line)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _phys(pkg, x):
    """numpy (N, 3, H, W) -> the physical (N, H, W, 4) device tensor."""
    return pkg.ops.as_phys(pkg.ops.to_nhwc(_dev(x)))


def _nchw(phys):
    """physical (N, H, W, 4) -> numpy (N, 4, H, W), the pad channel included."""
    return phys.cpu().numpy().transpose(0, 3, 1, 2)


def _images(shape, seed):
    n, h, w = shape
    return np.random.RandomState(seed).rand(n, 3, h, w).astype(np.float32)


# ------------------------------------------------------------------ pool
@pytest.mark.parametrize("shape", [(1, 64, 64), (3, 40, 32)])
def test_pool_matches_float64_and_its_adjoint_is_its_adjoint(pkg, shape):
    """The mean is formed in double and rounded once: |error| <= 2^-24 |mean| (+ the double sum's 2^-52).  adj(y) = y / 4 is
    exact, so <pool(x), y> and <x, adj(y)>, both in float64 on the read-back tensors, differ by the rounding of pool(x) alone:
    at most 2^-24 sum |pool(x)| |y|."""
    ops = pkg.ops
    n, h, w = shape
    x = (_images(shape, 1) * 4.0 - 2.0).astype(np.float32)
    xp = _phys(pkg, x)
    got = _nchw(ops.swd_pool(xp))
    assert got.shape == (n, 4, h // 2, w // 2) and (got[:, 3].view(np.int32) == 0).all()
    want = ref.pool_ref(x.astype(np.float64))
    err = np.abs(got[:, :3] - want)
    bound = 2.0 ** -24 * np.abs(want) * (1 + 2.0 ** -20) + 1e-45
    _note(f"pool     {shape}: max error / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    y = np.random.RandomState(2).randn(n, 3, h // 2, w // 2).astype(np.float32)
    adj = _nchw(ops.swd_pool_adjoint_add(_phys(pkg, y), torch.zeros_like(xp)))
    assert (adj[:, 3].view(np.int32) == 0).all()
    assert np.array_equal(adj[:, :3], np.repeat(np.repeat(y * np.float32(0.25), 2, axis=2), 2, axis=3))
    lhs = float((got[:, :3].astype(np.float64) * y).sum())
    rhs = float((x.astype(np.float64) * adj[:, :3]).sum())
    slack = 2.0 ** -24 * float((np.abs(got[:, :3]).astype(np.float64) * np.abs(y)).sum())
    _note(f"pool     {shape}: <pool x, y> - <x, adj y> = {lhs - rhs:.3e}  bound {slack:.3e}")
    assert abs(lhs - rhs) <= slack
    # it ADDS: values in [1, 2) make fine + coarse / 4 exact in double, so the fma's one rounding is float32(double sum)
    fine = (1.0 + _images(shape, 3)).astype(np.float32)
    coarse = (1.0 + _images((n, h // 2, w // 2), 4)).astype(np.float32)
    fp = _phys(pkg, fine)
    fp[..., 3] = 7.0
    added = _nchw(ops.swd_pool_adjoint_add(_phys(pkg, coarse), fp))
    up = np.repeat(np.repeat(coarse.astype(np.float64), 2, axis=2), 2, axis=3)
    assert np.array_equal(added[:, :3], (fine.astype(np.float64) + 0.25 * up).astype(np.float32))
    assert (added[:, 3] == 7.0).all()                                      # channel 3 is left alone
    with pytest.raises(RuntimeError, match="no coarser"):
        ops.swd_pool(torch.zeros(1, 16, 32, 4, device=DEV))
    with pytest.raises(RuntimeError, match="half-size"):
        ops.swd_pool_adjoint_add(torch.zeros(1, 16, 16, 4, device=DEV), torch.zeros(1, 32, 64, 4, device=DEV))


# ------------------------------------------------------------------ grid gather / scatter
def _scatter_ref(gdesc, shape, s, oy, ox):
    n, h, w = shape
    cy, cx = h // s, w // s
    out = np.zeros((n, 4, h, w), dtype=np.float32)
    g = gdesc.reshape(n, cy, cx, 3, 7, 7)
    for i in range(cy):
        for j in range(cx):
            out[:, :3, i * s + oy:i * s + oy + 7, j * s + ox:j * s + ox + 7] = g[:, i, j]
    return out


@pytest.mark.parametrize("shape,offsets", [((2, 16, 16), [(0, 0), (1, 1), (0, 1)]), ((3, 40, 24), [(1, 0)]),
                                           ((9, 256, 256), [(0, 2), (2, 0)]), ((16, 256, 256), [(5, 0)])])
def test_grid_gather_is_numpy_slicing_and_scatter_its_exact_adjoint(pkg, shape, offsets):
    """Offsets 0 and s - 7 both land inside their cell; 40 x 24 is non-square; at 9 and 16 images of 256 x 256 the cells grow
    to 9 and 12 and leave 4 rows and columns outside every cell."""
    ops = pkg.ops
    n, h, w = shape
    s = ops.swd_cell_side(n, h, w)
    assert s == {2: 8, 3: 8, 9: 9, 16: 12}[n]
    x = _images(shape, 5) - 0.5
    xp = _phys(pkg, x)
    rows = n * (h // s) * (w // s)
    gd = np.random.RandomState(6).randn(rows, 147).astype(np.float32)
    gd[0, 0] = -0.0
    for oy, ox in offsets:
        got = ops.swd_grid_gather(xp, s, oy, ox)
        assert tuple(got.shape) == (rows, 147)
        assert np.array_equal(got.cpu().numpy(), ref.grid_gather_ref(x, s, oy, ox))
        out = _nchw(ops.swd_grid_scatter(_dev(gd), shape, s, oy, ox))
        want = _scatter_ref(gd, shape, s, oy, ox)
        assert np.array_equal(out.view(np.int32), want.view(np.int32))     # bit for bit: every other pixel and channel 3 are +0.0
        # <gather(x), gd> = <x, scatter(gd)> follows from the two equalities above; the scale and the device scalar multiply in
        half = _nchw(ops.swd_grid_scatter(_dev(gd), shape, s, oy, ox, 0.25, torch.tensor(2.0, device=DEV)))
        assert np.array_equal(half, want * np.float32(0.5))
    with pytest.raises(RuntimeError, match="offset"):
        ops.swd_grid_gather(xp, s, s - 6, 0)
    with pytest.raises(RuntimeError, match="offset"):
        ops.swd_grid_scatter(_dev(gd), shape, s, 0, -1)
    with pytest.raises(RuntimeError, match="gdesc"):
        ops.swd_grid_scatter(_dev(gd[:-1]), shape, s, 0, 0) if rows > 1 else ops.swd_grid_scatter(_dev(gd.T), shape, s, 0, 0)


# ------------------------------------------------------------------ indexed sort
@pytest.mark.parametrize("n", [1, 2, 3, 45, 64, 65, 4097, 8192])
def test_sort_columns_indexed_is_a_stable_argsort(pkg, n):
    cols = 12                                                              # every kind of column twice
    m = _sort_input(n, cols, n)
    want = torch.sort(torch.from_numpy(m), dim=0, stable=True)
    keys, rows = pkg.ops.sort_columns_indexed(_dev(m))                     # row-major
    assert keys.is_contiguous() and rows.is_contiguous() and rows.dtype == torch.int32
    assert np.array_equal(keys.cpu().numpy(), want.values.numpy())
    assert np.array_equal(rows.cpu().numpy(), want.indices.numpy())
    tr = _dev(m.T).t()                                                     # the layout swd_project hands over
    keys_t, rows_t = pkg.ops.sort_columns_indexed(tr)
    assert keys_t.stride() == tr.stride() == rows_t.stride()
    assert np.array_equal(keys_t.cpu().numpy(), want.values.numpy())
    assert np.array_equal(rows_t.cpu().numpy(), want.indices.numpy())


def test_sort_columns_indexed_with_a_nan_key_and_with_too_many_rows(pkg):
    m = _sort_input(1000, 12, 78)
    m[123, 5] = np.nan
    keys, rows = pkg.ops.sort_columns_indexed(_dev(m))
    torch.cuda.synchronize()
    k, r = keys.cpu().numpy(), rows.cpu().numpy()
    others = [j for j in range(12) if j != 5]
    want = torch.sort(torch.from_numpy(m[:, others]), dim=0, stable=True)
    assert np.array_equal(k[:, others], want.values.numpy()) and np.array_equal(r[:, others], want.indices.numpy())
    assert np.array_equal(np.sort(r[:, 5]), np.arange(1000))               # still a permutation of the rows ...
    assert np.array_equal(k[:, 5], m[r[:, 5], 5], equal_nan=True)          # ... and the keys are still theirs
    x = torch.zeros(8193, 2, device=DEV)
    with pytest.raises(RuntimeError, match="8192"):
        pkg.ops.sort_columns_indexed(x)
    lib = pkg._native.lib()
    out, idx = torch.full_like(x, 5.0), torch.full((8193, 2), 5, dtype=torch.int32, device=DEV)
    assert lib.vcg_sort_columns_indexed(x.data_ptr(), out.data_ptr(), idx.data_ptr(), 8193, 2, 2, 1, None) != 0
    assert b"8192" in lib.vcg_last_error()
    torch.cuda.synchronize()
    assert (out == 5.0).all() and (idx == 5).all()                          # nothing was launched


# ------------------------------------------------------------------ pair loss, transposed projection
_PAIR = {}


def _pair_case(pkg, n):
    """Sorted projections of two random sets with ties between them, the device's pair loss on them — computed once."""
    if n not in _PAIR:
        ops = pkg.ops
        rng = np.random.RandomState(n)
        a = rng.randn(n, 128).astype(np.float32)
        b = rng.randn(n, 128).astype(np.float32)
        b[:, 3] = a[:, 3]                                                  # a whole direction of exact ties: sign 0
        b[: max(1, n // 5), 7] = a[: max(1, n // 5), 7]
        ka, ra = ops.sort_columns_indexed(_dev(a.T).t())
        kb = ops.sort_columns(_dev(b.T).t())
        out, gproj, total = ops.swd_pair_loss(ka, kb, ra)
        _PAIR[n] = (ka, kb, ra, out, gproj, total)
    return _PAIR[n]


@pytest.mark.parametrize("n", [45, 8192])
def test_pair_loss_value_and_signed_gradient(pkg, n):
    """The value against the float64 mean of the device's own sorted inputs within 1e-4 relative, the bound tests/test_gpu_swd.py
    holds the distance to; gproj is sign(a - b) scattered by the permutation, exactly."""
    ka, kb, ra, out, gproj, total = _pair_case(pkg, n)
    a64, b64, r = ka.cpu().numpy().astype(np.float64), kb.cpu().numpy().astype(np.float64), ra.cpu().numpy()
    want = np.abs(a64 - b64).mean()
    got = float(out)
    _note(f"pair     n={n:5d}: device {got:.8f} float64 {want:.8f} relative error {abs(got - want) / want:.3e}  bound 1.000e-04")
    assert abs(got - want) <= 1e-4 * want
    assert float(total) == pytest.approx(want, rel=1e-12) and got == float(np.float32(float(total)))
    exp = np.full((128, n), 9.0, dtype=np.float32)
    np.put_along_axis(exp, r.T.astype(np.int64), np.sign(a64 - b64).T.astype(np.float32), axis=1)
    g = gproj.cpu().numpy()
    assert gproj.is_contiguous() and np.array_equal(g, exp)
    assert (g[3] == 0).all() and set(np.unique(g)) == {-1.0, 0.0, 1.0}
    # a second level accumulates into the running double with its weight
    out2, gproj2, total2 = pkg.ops.swd_pair_loss(ka, kb, ra, 0.5, total.clone())
    assert torch.equal(gproj2, gproj)
    assert float(total2) == pytest.approx(1.5 * want, rel=1e-12) and float(out2) == float(np.float32(float(total2)))


@pytest.mark.parametrize("n", [45, 8192])
def test_transposed_projection_matches_float64(pkg, n):
    """gdesc = gproj^T dirs^T is vcg_swd_project with the roles swapped, K = 128 terms: |error| <= 128 * 2^-24 *
    (|gproj|^T @ |dirs|^T); n = 45 is under one 64-wide tile, 147 rows are two tiles and 19."""
    gproj = _pair_case(pkg, n)[4]
    dirs = pkg.Losses.SlicedWassersteinLoss(seed=3).directions(DEV, 0)
    got = pkg.ops.swd_project(dirs, gproj).t()
    assert tuple(got.shape) == (n, 147) and got.is_contiguous()
    g64, d64 = gproj.cpu().numpy().astype(np.float64), dirs.cpu().numpy().astype(np.float64)
    want = g64.T @ d64.T
    bound = 128 * 2.0 ** -24 * (np.abs(g64).T @ np.abs(d64).T)
    err = np.abs(got.cpu().numpy() - want)
    _note(f"project^T n={n:5d}: max error / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert (err <= bound).all()


# ------------------------------------------------------------------ unit columns
def test_unit_columns_and_the_directions_of_a_step(pkg):
    ops = pkg.ops
    gauss = ops.randn((147, 128), DEV, seed=9, offset=0)
    u = ops.swd_unit_columns(gauss)
    assert torch.equal(u, ops.swd_unit_columns(gauss))
    norms = np.sqrt((u.cpu().numpy().astype(np.float64) ** 2).sum(axis=0))
    _note(f"unit     147 x 128: max | norm - 1 | {np.abs(norms - 1).max():.3e}  bound {2.0 ** -22:.3e}")
    assert np.abs(norms - 1).max() <= 2.0 ** -22
    ratio = (u / gauss).cpu().numpy()
    assert np.abs(ratio / ratio[0:1] - 1).max() < 1e-6                      # one factor per column
    odd = ops.swd_unit_columns(ops.randn((5, 3), DEV, seed=1))
    assert np.abs(np.sqrt((odd.cpu().numpy().astype(np.float64) ** 2).sum(axis=0)) - 1).max() <= 2.0 ** -22
    loss = pkg.Losses.SlicedWassersteinLoss(seed=4)
    d0, d1 = loss.directions(DEV, 0), loss.directions(DEV, 1)
    assert torch.equal(d0, loss.directions(DEV)) and torch.equal(d0, pkg.Losses.SlicedWassersteinLoss(seed=4).directions(DEV, 0))
    assert not torch.equal(d0, pkg.Losses.SlicedWassersteinLoss(seed=5).directions(DEV, 0))
    flat0, flat1 = d0.cpu().numpy().ravel(), d1.cpu().numpy().ravel()
    assert abs(np.corrcoef(flat0[4:], flat1[:-4])[0, 1]) < 0.05 and abs(np.corrcoef(flat0, flat1)[0, 1]) < 0.05     # disjoint draws


# ------------------------------------------------------------------ end to end
_E2E = {}


def _e2e_case(pkg, shape, levels):
    """Images, plan, the device's value and gradient (twice), the float64 and float32 restatements — computed once per shape."""
    key = (shape, levels)
    if key not in _E2E:
        ops = pkg.ops
        n, h, w = shape
        a, b = _images(shape, 11), _images(shape, 12)
        b = (0.7 * b + 0.1).astype(np.float32)
        loss = pkg.Losses.SlicedWassersteinLoss(levels=levels, seed=21)
        plan = ops.SwdPlan(loss.offsets(n, h, w, 3), loss.directions(DEV, 3))
        runs = []
        for _ in range(2):
            ga = ops.to_nhwc(_dev(a)).requires_grad_(True)
            tb = ops.to_nhwc(_dev(b))
            v = ops.swd_loss(ga, tb, levels, plan)
            v.backward()
            assert tb.grad is None
            runs.append((v.detach().cpu().numpy().copy(), ops.to_nchw_contiguous(ga.grad).cpu().numpy()))
        dirs = plan.directions.cpu()
        refs = {}
        for dtype in (torch.float64, torch.float32):
            x = torch.from_numpy(a).to(dtype).requires_grad_(True)
            val = ref.swd_loss_ref(x, torch.from_numpy(b), levels, plan.offsets, dirs, dtype)
            val.backward()
            refs[dtype] = (float(val.detach()), x.grad.to(torch.float64).numpy())
        _E2E[key] = (a, b, plan, runs, refs)
    return _E2E[key]


def _chain(pkg, a, b, levels, plan, g):
    """ops.swd_loss written out in its stage calls: -> (value, gradient as a physical map)."""
    ops = pkg.ops
    la, lb = _phys(pkg, a), _phys(pkg, b)
    n_img = a.shape[0]
    total, kept = None, []
    for k in range(levels):
        if k:
            la, lb = ops.swd_pool(la), ops.swd_pool(lb)
        hk, wk = la.shape[1:3]
        s = ops.swd_cell_side(n_img, hk, wk)
        oy, ox = plan.offsets[k]
        ka, ra = ops.sort_columns_indexed(ops.swd_project(ops.swd_grid_gather(la, s, oy, ox), plan.directions))
        kb = ops.sort_columns(ops.swd_project(ops.swd_grid_gather(lb, s, oy, ox), plan.directions))
        out, gproj, total = ops.swd_pair_loss(ka, kb, ra, 1.0 / levels, total)
        kept.append((gproj, hk, wk, s, oy, ox))
    coarser = None
    for gproj, hk, wk, s, oy, ox in reversed(kept):
        gdesc = ops.swd_project(plan.directions, gproj).t()
        m = ops.swd_grid_scatter(gdesc, (n_img, hk, wk), s, oy, ox, 1.0 / (gproj.shape[1] * 128 * levels), g)
        if coarser is not None:
            ops.swd_pool_adjoint_add(coarser, m)
        coarser = m
    return out, coarser


@pytest.mark.parametrize("shape,levels", E2E)
def test_swd_loss_is_its_stage_calls_and_reproducible(pkg, shape, levels):
    a, b, plan, runs, _ = _e2e_case(pkg, shape, levels)
    (v0, g0), (v1, g1) = runs
    assert v0.dtype == np.float32 and v0.shape == () and v0.tobytes() == v1.tobytes() and np.array_equal(g0, g1)
    out, gmap = _chain(pkg, a, b, levels, plan, torch.ones((), device=DEV))
    assert out.cpu().numpy().tobytes() == v0.tobytes()
    gm = _nchw(gmap)
    assert np.array_equal(gm[:, :3].view(np.int32), g0.view(np.int32)) and (gm[:, 3].view(np.int32) == 0).all()
    assert np.isfinite(g0).all() and (g0 != 0).any()
    if levels == 1:                                                        # pixels in no patch get exactly 0
        s = pkg.ops.swd_cell_side(*shape)
        oy, ox = plan.offsets[0]
        mask = _scatter_ref(np.ones((shape[0] * (shape[1] // s) * (shape[2] // s), 147), np.float32), shape, s, oy, ox)[:, :3] != 0
        assert (g0[~mask].view(np.int32) == 0).all() and mask.any() and (~mask).any()


@pytest.mark.parametrize("shape,levels", E2E)
def test_swd_loss_value_against_float64(pkg, shape, levels):
    """The sorted pairing is 1-Lipschitz in the sup norm of the projections, so the value moves by at most the largest projection
    error: 148 * 2^-24 * max (|desc| @ |dirs|) — the 147-term fp32 dot product of test_project_matches_float64 plus the one
    rounding of a pooled pixel — and the mean itself is held to the distance bound, 1e-4 relative."""
    a, b, plan, runs, refs = _e2e_case(pkg, shape, levels)
    want = refs[torch.float64][0]
    d64 = np.abs(plan.directions.cpu().numpy().astype(np.float64))
    proj = 0.0
    la, lb = a.astype(np.float64), b.astype(np.float64)
    for k in range(levels):
        if k:
            la, lb = ref.pool_ref(la), ref.pool_ref(lb)
        s = ref.cell_side(shape[0], la.shape[2], la.shape[3])
        for lv in (la, lb):
            proj = max(proj, 148 * 2.0 ** -24 * float((np.abs(ref.grid_gather_ref(lv, s, *plan.offsets[k])) @ d64).max()))
    got = float(runs[0][0])
    bound = proj + 1e-4 * want
    _note(f"swd_loss {shape} levels {levels}: device {got:.8f} float64 {want:.8f} error {abs(got - want):.3e}  bound {bound:.3e}")
    assert want > 0 and abs(got - want) <= bound


def test_swd_loss_of_a_set_with_itself_is_exactly_zero(pkg):
    ops = pkg.ops
    a = _images((1, 64, 64), 31)
    loss = pkg.Losses.SlicedWassersteinLoss(levels=3, seed=2)
    ga = ops.to_nhwc(_dev(a)).requires_grad_(True)
    v = loss(ga, ops.to_nhwc(_dev(a.copy())))
    v.backward()
    assert loss.step == 1
    assert v.detach().cpu().numpy().view(np.int32) == 0
    assert (ops.to_nchw_contiguous(ga.grad).cpu().numpy().view(np.int32) == 0).all()
    with pytest.raises(RuntimeError, match="which have 2"):
        pkg.Losses.SlicedWassersteinLoss(levels=3)(torch.zeros(1, 3, 32, 32, device=DEV), torch.zeros(1, 3, 32, 32, device=DEV))
    with torch.no_grad():                                                   # validation: no graph, same value
        w = pkg.Losses.SlicedWassersteinLoss(levels=3, seed=2)(ga, ops.to_nhwc(_dev(a.copy())))
    assert float(w) == 0.0 and not w.requires_grad


@pytest.mark.parametrize("shape,levels", E2E)
def test_gradient_against_float64(pkg, shape, levels):
    """<g, v> along 8 random unit directions v against the float64 autograd gradient of the restatement.  The gradient is piecewise
    constant and near-ties flip signs, so no bound can be derived: the device is allowed 4 x what the SAME restatement run in
    float32 on the CPU is off by (the same flips, plus the MFMA's summation order).  Measured (profiles/swd_loss_error.txt), device |
    float32 restatement: 2x16x16 2.2e-10 | 2.2e-10, 3x40x24 7.7e-11 | 4.7e-11, 1x64x64 (3 levels) 3.2e-11 | 1.6e-11, 9x256x256
    3.7e-13 | 4.0e-13."""
    a, b, plan, runs, refs = _e2e_case(pkg, shape, levels)
    g_dev, g64, g32 = runs[0][1].astype(np.float64), refs[torch.float64][1], refs[torch.float32][1]
    rng = np.random.RandomState(99)
    e_dev = e_ref = 0.0
    for _ in range(8):
        v = rng.randn(*g64.shape)
        v /= np.sqrt((v ** 2).sum())
        e_dev = max(e_dev, abs(float((g_dev * v).sum() - (g64 * v).sum())))
        e_ref = max(e_ref, abs(float((g32 * v).sum() - (g64 * v).sum())))
    norm = float(np.sqrt((g64 ** 2).sum()))
    _note(f"gradient {shape} levels {levels}: device {e_dev:.3e} float32 restatement {e_ref:.3e} (|g64| {norm:.3e})  bound {4 * e_ref:.3e}")
    assert e_dev <= 4 * e_ref


# ------------------------------------------------------------------ the models
SEED, LR = 20261020, 2e-4


def _twins(device, make, configure):
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


def _batch(pkg, n, size):
    return {"x": pkg.ops.rand_uniform((n, 3, size, size), DEV, seed=SEED, offset=0),
            "y": pkg.ops.rand_uniform((n, 3, size, size), DEV, seed=SEED, offset=1 << 22)}


def _same_bits(ma, mb):
    assert list(ma) == list(mb), f"metric keys {list(ma)} vs {list(mb)}"
    for k in ma:
        assert np.float64(ma[k]).tobytes() == np.float64(mb[k]).tobytes(), f"{k}: {ma[k]!r} vs {mb[k]!r}"


def _step(pkg, model, batch):
    pkg.ops.manual_seed(SEED)
    return model.training_step(batch)


def test_cyclevae_step_with_the_term_off_on_and_resumed(pkg, tmp_path):
    """cyclevae unpaired, 64 x 64, batch 2: lambda_swd = 0 is the model configured without the keyword bit for bit; with
    lambda_swd = 1 loss_swd is reported, finite, part of G_loss, every parameter has a finite gradient and the eps stream is
    consumed as without the term; a checkpoint saved after step 1 and resumed gives step 2 bit for bit."""
    N, utils = pkg.Networks, pkg.utils
    make = lambda: N.CycleVAE(latent_dim=64, paired=False)              # noqa: E731
    plain, zero, on, resumed = _twins(DEV, make, [{}, {"lambda_swd": 0.0}, {"lambda_swd": 1.0, "swd_seed": 7},
                                                   {"lambda_swd": 1.0, "swd_seed": 99}])
    batch = _batch(pkg, 2, 64)
    m_plain, m_zero = _step(pkg, plain, batch), _step(pkg, zero, batch)
    eps_after = pkg.ops._RNG["offset"]
    assert "loss_swd" not in m_zero and zero.swd_term is None
    _same_bits(m_plain, m_zero)
    assert torch.equal(plain.optimizer.flat_param, zero.optimizer.flat_param)
    m_on = _step(pkg, on, batch)
    assert pkg.ops._RNG["offset"] == eps_after                             # the term draws from a stream of its own
    assert list(m_on) == list(m_plain) + ["loss_swd"] and np.isfinite(m_on["loss_swd"]) and m_on["loss_swd"] > 0
    assert m_on["loss_cycle"] == m_plain["loss_cycle"] and m_on["loss_kl"] == m_plain["loss_kl"]
    expect = m_plain["G_loss"] + m_on["loss_swd"]
    assert abs(m_on["G_loss"] - expect) <= 1e-5 * abs(expect)
    assert on.swd_term[1].step == 2                                        # swd(G(x), y) and swd(F(y), x)
    for name, p in on.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert not torch.equal(on.optimizer.flat_param, plain.optimizer.flat_param)
    v = on.validation_step(batch)
    assert "loss_swd" in v and np.isfinite(v["loss_swd"]) and on.swd_term[1].step == 4
    args = type("Args", (), {})()
    utils.save_checkpoint(on, 0, m_on["G_loss"], args, tmp_path / "c.pth")
    saved_rng = dict(pkg.ops._RNG)
    step2 = on.training_step(batch)
    pkg.ops.manual_seed(1)                                                 # the loader restores the eps stream too
    utils.load_checkpoint(resumed, tmp_path / "c.pth", DEV)
    assert (resumed.swd_term[1].seed, resumed.swd_term[1].step) == (7, 4) and dict(pkg.ops._RNG) == saved_rng
    _same_bits(step2, resumed.training_step(batch))
    assert torch.equal(on.optimizer.flat_param, resumed.optimizer.flat_param)


def test_cycleaegan_step_leaves_the_discriminators_alone(pkg):
    """cycleaegan unpaired, batch 2, at 256 x 256 — the one size the discriminators take: with lambda_swd = 1 the generators'
    gradients are finite and differ from the twin's, the discriminators' gradients and losses are the twin's bit for bit."""
    N = pkg.Networks
    on, off = _twins(DEV, lambda: N.CycleAEGAN(paired=False), [{"lambda_swd": 1.0, "swd_levels": 3}, {}])
    batch = _batch(pkg, 2, 256)
    m_on, m_off = _step(pkg, on, batch), _step(pkg, off, batch)
    assert list(m_on) == list(m_off) + ["loss_swd"] and np.isfinite(m_on["loss_swd"]) and m_on["loss_swd"] > 0
    assert m_on["D_loss"] == m_off["D_loss"] and m_on["loss_cycle"] == m_off["loss_cycle"]
    expect = m_off["G_loss"] + m_on["loss_swd"]
    assert abs(m_on["G_loss"] - expect) <= 1e-5 * abs(expect)
    p_on, p_off = dict(on.named_parameters()), dict(off.named_parameters())
    differ = 0
    for name, p in p_on.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        if name.startswith(("DX.", "DY.")):
            assert torch.equal(p.grad, p_off[name].grad), name
        else:
            differ += int(not torch.equal(p.grad, p_off[name].grad))
    assert differ > 0
    assert torch.equal(on.optimizer_D.flat_param, off.optimizer_D.flat_param)
