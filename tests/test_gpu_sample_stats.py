"""GPU: the three kernels of the sampling translator (csrc/sample_stats.hip) — the broadcast reparameterisation against
ops.reparameterize and vcg_randn bit for bit, the running statistics against float64 and against themselves under every chunking,
the spread map against float64.

Outputs are prefilled with NaN words and followed by a guard band of sentinel bytes (tests/test_gpu_translate.py's scheme): an
element a kernel does not write, or one it writes past the end, fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64
SENTINEL = 0x5A


class Out:
    """`nbytes` of output prefilled with 0xFF bytes (NaN as fp32, 255 as uint8), then GUARD sentinel bytes."""

    def __init__(self, nbytes, fill=0xFF):
        self.n = nbytes
        self.buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
        self.buf[:nbytes] = fill
        self.buf[nbytes:] = SENTINEL

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def get(self, dtype, shape):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == SENTINEL).all()), "the kernel wrote past the end of its output"
        return self.buf[:self.n].view(dtype).reshape(shape).cpu().numpy()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ vcg_reparam_many_fwd
N, K = 2, 5
LATENTS = [(4, 1, 1), (64, 2, 3), (6, 2, 2)]           # per = 4, 64 * 2 * 3, 8 * 2 * 2 (latent_dim 6 at pitch 8)
CHUNKINGS = [[(0, 5)], [(0, 2), (2, 3)], [(j, 1) for j in range(5)]]
SEED, OFFSET = 20261019, 123457


def _latent_inputs(c, h, w, seed):
    rng = np.random.RandomState(seed)
    mu = rng.randn(N, c, h, w).astype(np.float32)
    lv = (2.0 * rng.randn(N, c, h, w)).astype(np.float32)
    eps = rng.randn(N, K, c, h, w).astype(np.float32)
    return mu, lv, eps


def _many(pkg, mu_p, lv_p, eps_p, first, k, per, temperature=1.0, seed=SEED, offset=OFFSET):
    """The ABI call on physical buffers -> (z, eps used) as (N, k, per) host arrays."""
    z, used = Out(N * k * per * 4), Out(N * k * per * 4)
    pkg._native.check(pkg._native.lib().vcg_reparam_many_fwd(_p(mu_p), _p(lv_p), _p(eps_p), used.ptr(), z.ptr(), N, K, first, k, per,
                                                             temperature, seed, offset, None), "vcg_reparam_many_fwd")
    return z.get(torch.float32, (N, k, per)), used.get(torch.float32, (N, k, per))


@pytest.mark.parametrize("c,h,w", LATENTS)
def test_reparam_many_with_explicit_eps_is_reparameterize_bit_for_bit(pkg, c, h, w):
    ops = pkg.ops
    mu, lv, eps = _latent_inputs(c, h, w, 11 + c)
    MU, LV = ops.to_nhwc(torch.from_numpy(mu).to(DEV)), ops.to_nhwc(torch.from_numpy(lv).to(DEV))
    assert ops.phys_of(MU)[0].numel() == {4: 4, 64: 64 * 2 * 3, 6: 8 * 2 * 2}[c]
    before = dict(ops._RNG)
    z, used = ops.reparameterize_many(MU, LV, K, eps=torch.from_numpy(eps).to(DEV))
    assert dict(ops._RNG) == before, "injected eps must not move the stream"
    assert tuple(z.shape) == (N * K, c, h, w) and ops.is_nhwc_view(z)
    z, used = z.contiguous().cpu().numpy().reshape(N, K, c, h, w), used.contiguous().cpu().numpy().reshape(N, K, c, h, w)
    assert np.array_equal(_bits(used), _bits(eps))
    for n in range(N):
        for j in range(K):
            want, _ = ops.reparameterize(MU[n:n + 1], LV[n:n + 1], ops.to_nhwc(torch.from_numpy(eps[n, j][None]).to(DEV)))
            assert np.array_equal(_bits(z[n, j]), _bits(want.contiguous().cpu().numpy()[0])), (n, j)
    # a chunk in the middle: the same samples
    zc, _ = ops.reparameterize_many(MU, LV, K, first=1, count=3, eps=torch.from_numpy(eps[:, 1:4]).to(DEV))
    assert np.array_equal(_bits(zc.contiguous().cpu().numpy().reshape(N, 3, c, h, w)), _bits(z[:, 1:4]))


@pytest.mark.parametrize("c,h,w", LATENTS)
def test_reparam_many_draws_do_not_depend_on_the_chunking_and_are_vcg_randn(pkg, c, h, w):
    ops = pkg.ops
    mu, lv, _ = _latent_inputs(c, h, w, 23 + c)
    MU, LV = ops.phys_of(ops.to_nhwc(torch.from_numpy(mu).to(DEV))), ops.phys_of(ops.to_nhwc(torch.from_numpy(lv).to(DEV)))
    per = MU[0].numel()
    results = []
    for plan in CHUNKINGS:
        parts = [_many(pkg, MU, LV, None, first, k, per) for first, k in plan]
        results.append((np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)))
    for z, e in results[1:]:
        assert np.array_equal(_bits(z), _bits(results[0][0])) and np.array_equal(_bits(e), _bits(results[0][1]))
    # the documented layout: sample (n, j) is what vcg_randn writes for (seed, offset + (n K + j) per / 4)
    want = np.stack([np.stack([ops.randn((per,), DEV, SEED, OFFSET + (n * K + j) * per // 4).cpu().numpy() for j in range(K)])
                     for n in range(N)])
    assert np.array_equal(_bits(results[0][1]), _bits(want))
    assert len(np.unique(want)) > 0.99 * want.size                         # no two samples share their noise
    # ... and the explicit path fed with it gives the drawn path's z
    z, _ = _many(pkg, MU, LV, torch.from_numpy(want).to(DEV), 0, K, per)
    assert np.array_equal(_bits(z), _bits(results[0][0]))
    assert np.isfinite(results[0][0]).all()


def test_reparameterize_many_reserves_the_stream_once_per_batch(pkg):
    ops = pkg.ops
    mu, lv, _ = _latent_inputs(6, 2, 2, 5)
    MU, LV = ops.to_nhwc(torch.from_numpy(mu).to(DEV)), ops.to_nhwc(torch.from_numpy(lv).to(DEV))
    per = 8 * 2 * 2
    ops.manual_seed(77)
    ops._RNG["offset"] = 40
    whole, _ = ops.reparameterize_many(MU, LV, K)
    assert ops._RNG["offset"] == 40 + N * K * per // 4
    ops._RNG["offset"] = 40
    off = ops.reserve_eps_many(MU, K)
    assert off == 40 and ops._RNG["offset"] == 40 + N * K * per // 4
    parts = [ops.reparameterize_many(MU, LV, K, first, k, seed_offset=off)[0] for first, k in CHUNKINGS[1]]
    assert ops._RNG["offset"] == 40 + N * K * per // 4                     # the chunks moved nothing
    got = torch.cat([p.contiguous().view(N, -1, 6, 2, 2) for p in parts], dim=1)
    assert torch.equal(got.view(torch.int32), whole.contiguous().view(N, K, 6, 2, 2).view(torch.int32))
    with pytest.raises(RuntimeError, match="seed_offset"):
        ops.reparameterize_many(MU, LV, K, first=2, count=3)
    ops.manual_seed(78)
    other, _ = ops.reparameterize_many(MU, LV, K)
    assert not torch.equal(other.contiguous(), whole.contiguous())


def test_reparam_many_temperature_and_clamp(pkg):
    rng = np.random.RandomState(3)
    per = 64 * 2 * 3
    mu = rng.randn(N, per).astype(np.float32)
    mu[0, :4] = [-0.0, 0.0, 1e-30, -3.5]
    lv = (2.0 * rng.randn(N, per)).astype(np.float32)
    lv[1, :6] = [50.0, -50.0, 10.0, -10.0, 10.5, -1e30]
    eps = rng.randn(N, K, per).astype(np.float32)
    MU, LV, EPS = (torch.from_numpy(a).to(DEV) for a in (mu, lv, eps))
    for e in (EPS, None):
        z, _ = _many(pkg, MU, LV, e, 0, K, per, temperature=0.0)
        assert np.array_equal(_bits(z), _bits(np.broadcast_to(mu[:, None], (N, K, per)))), "temperature 0 must give mu's own bits"
    z, _ = _many(pkg, MU, LV, EPS, 0, K, per)
    zc, _ = _many(pkg, MU, torch.from_numpy(np.clip(lv, -10, 10)).to(DEV), EPS, 0, K, per)
    assert np.array_equal(_bits(z), _bits(zc)), "lv outside [-10, 10] must be clamped"
    sd = np.exp(0.5 * np.clip(lv.astype(np.float64), -10, 10))[:, None]
    for t in (1.0, 0.5, 2.0):
        z, _ = _many(pkg, MU, LV, EPS, 0, K, per, temperature=t)
        want = mu.astype(np.float64)[:, None] + t * eps.astype(np.float64) * sd
        # three fp32 roundings of the product and the sum, expf within a few ulp
        assert np.all(np.abs(z - want) <= 8 * 2.0 ** -24 * (np.abs(mu)[:, None] + np.abs(t * eps * sd))), t


# ------------------------------------------------------------------ vcg_sample_accumulate
KA = 7
ACC_BOUND = KA * 2.0 ** -21          # at most eight fp32 roundings of quantities <= 1 per update, KA updates
ACC_CHUNKINGS = [[7], [3, 4], [1] * 7]
_ACC_CACHE = {}


def _acc_case(pixels):
    """(y (2, KA, pixels, 4) fp32, float64 mean and unbiased variance of clamp(y[..., :3], 0, 1), which elements are constant across
    the samples), made once per size."""
    if pixels not in _ACC_CACHE:
        rng = np.random.RandomState(100 + pixels)
        y = (rng.rand(2, KA, pixels, 4) * 1.4 - 0.2).astype(np.float32)
        y[0, :, ::5, 0] = y[0, :1, ::5, 0]                                 # image 0: constant across the samples, inside, below and
        y[0, :, ::7, 1] = -0.1                                             # above the clamp (with one pixel: all of image 0)
        y[0, :, ::3, 2] = 1.15
        y[..., 3] = np.nan                                                 # the pad channel is not looked at
        x = np.clip(y[..., :3].astype(np.float64), 0.0, 1.0)
        assert (y[..., :3] < 0).any() and (y[..., :3] > 1).any()          # the clamp binds
        _ACC_CACHE[pixels] = (y, x.mean(axis=1), x.var(axis=1, ddof=1), (x == x[:, :1]).all(axis=1))
        for a in _ACC_CACHE[pixels]:
            a.setflags(write=False)
    return _ACC_CACHE[pixels]


def _accumulate(pkg, y, sizes, fill):
    n, _, pixels, _ = y.shape
    mean, m2 = Out(n * pixels * 16, fill), Out(n * pixels * 16, fill)
    seen = 0
    for k in sizes:
        chunk = torch.from_numpy(y[:, seen:seen + k].copy()).to(DEV)
        pkg._native.check(pkg._native.lib().vcg_sample_accumulate(_p(chunk), mean.ptr(), m2.ptr(), n, k, seen, pixels, None),
                          "vcg_sample_accumulate")
        seen += k
    return mean.get(torch.float32, (n, pixels, 4)), m2.get(torch.float32, (n, pixels, 4))


@pytest.mark.parametrize("pixels", [48 * 40, 1])
def test_accumulate_is_welford_whatever_the_chunking(pkg, pixels):
    y, mean64, var64, const = _acc_case(pixels)
    got = [_accumulate(pkg, y, sizes, 0xFF) for sizes in ACC_CHUNKINGS]
    mean, m2 = got[0]
    for other_mean, other_m2 in got[1:]:
        assert np.array_equal(_bits(other_mean), _bits(mean)) and np.array_equal(_bits(other_m2), _bits(m2))
    zeroed = _accumulate(pkg, y, [3, 4], 0x00)                              # dirty (NaN) buffers above, cleared ones here
    assert np.array_equal(_bits(zeroed[0]), _bits(mean)) and np.array_equal(_bits(zeroed[1]), _bits(m2))
    assert np.array_equal(_bits(mean[..., 3]), np.zeros((2, pixels), np.uint32)), "channel 3 of mean must be +0"
    assert np.array_equal(_bits(m2[..., 3]), np.zeros((2, pixels), np.uint32)), "channel 3 of m2 must be +0"
    e_mean = float(np.abs(mean[..., :3] - mean64).max())
    e_var = float(np.abs(m2[..., :3].astype(np.float64) / (KA - 1) - var64).max())
    print(f"accumulate pixels={pixels} K={KA}: max |mean - fp64| {e_mean:.3e}, max |m2 / (K - 1) - fp64| {e_var:.3e}, bound {ACC_BOUND:.3e}")
    assert e_mean <= ACC_BOUND and e_var <= ACC_BOUND
    assert const.sum() >= 1 and (~const).sum() >= 1
    assert np.array_equal(_bits(m2[..., :3][const]), np.zeros(int(const.sum()), np.uint32)), "constant elements must have m2 == +0"
    assert (m2[..., :3] >= 0).all()


def test_sample_accumulate_wrapper_folds_in_place(pkg):
    ops = pkg.ops
    y = _acc_case(48 * 40)[0]
    want_mean, want_m2 = _accumulate(pkg, y, [7], 0xFF)
    yy = np.where(np.isnan(y), 0, y).reshape(2, KA, 48, 40, 4)
    mean = ops.logical_of(torch.full((2, 48, 40, 4), float("nan"), device=DEV), 3)
    m2 = ops.logical_of(torch.full((2, 48, 40, 4), float("nan"), device=DEV), 3)
    seen = 0
    for k in (3, 4):
        chunk = torch.from_numpy(np.ascontiguousarray(yy[:, seen:seen + k]).reshape(2 * k, 48, 40, 4)).to(DEV)
        ops.sample_accumulate(ops.logical_of(chunk, 3), mean, m2, k, seen)
        seen += k
    assert np.array_equal(_bits(ops.phys_of(mean).cpu().numpy().reshape(2, -1, 4)), _bits(want_mean))
    assert np.array_equal(_bits(ops.phys_of(m2).cpu().numpy().reshape(2, -1, 4)), _bits(want_m2))
    with pytest.raises(RuntimeError, match="sample"):
        ops.sample_accumulate(ops.logical_of(chunk, 3), mean, m2, 3, 0)    # 8 images are not 3 samples of 2 frames


# ------------------------------------------------------------------ vcg_spread_display_hw
COUNT, GAIN = 7, 2.0
SPREAD_SEED = 1


def _spread_m2(n, hp, wp, seed=SPREAD_SEED):
    rng = np.random.RandomState(seed + hp * wp)
    m2 = (rng.rand(n, hp, wp, 4) * 1.5).astype(np.float32)                 # s up to ~0.5: gain 2 reaches the saturation
    m2[:, ::6, ::5, :3] = 0.0                                              # pixels on which every sample agreed
    m2[:, 1::9, 2::7, :3] = 4.0                                            # above anything [0, 1] samples can give: saturates
    m2[..., 3] = np.nan
    return m2


def spread_ref(m2, window, count=COUNT, gain=GAIN):
    """float64: (s, the value whose floor is the uint8 map, per-image mean of s)."""
    top, left, h, w = window
    v = m2[:, top:top + h, left:left + w, :3].astype(np.float64)
    s = np.sqrt(v.sum(axis=3) / (3.0 * (count - 1)))
    return s, 255.0 * np.minimum(1.0, gain * s) + 0.5, s.mean(axis=(1, 2))


def _spread(pkg, m2, window, count=COUNT, gain=GAIN):
    lib = pkg._native.lib()
    n, hp, wp, _ = m2.shape
    top, left, h, w = window
    need = lib.vcg_spread_workspace(n, h, w)
    assert need == (n * ((h + 15) // 16) * ((w + 15) // 16) * 8 + 15) // 16 * 16
    f32, u8, res, ws = Out(n * h * w * 4), Out(n * h * w), Out(n * 4), Out(need)
    src = torch.from_numpy(m2).to(DEV)
    pkg._native.check(lib.vcg_spread_display_hw(_p(src), count, gain, f32.ptr(), u8.ptr(), res.ptr(), n, hp, wp, top, left, h, w,
                                                ws.ptr(), need, None), "vcg_spread_display_hw")
    ws.get(torch.uint8, (need,))                                           # the workspace's guard band
    return f32.get(torch.float32, (n, h, w)), u8.get(torch.uint8, (n, h, w)), res.get(torch.float32, (n,))


@pytest.mark.parametrize("hp,wp,window", [(48, 64, None), (48, 64, (3, 5, 20, 37)), (32, 32, None)])
def test_spread_against_float64(pkg, hp, wp, window):
    n = 2
    window = window or (0, 0, hp, wp)
    m2 = _spread_m2(n, hp, wp)
    s64, v64, mean64 = spread_ref(m2, window)
    f32, u8, res = _spread(pkg, m2, window)
    want32 = s64.astype(np.float32)
    ulps = np.abs(f32.astype(np.float64) - want32) / np.spacing(np.maximum(want32, np.float32(1e-30))).astype(np.float64)
    print(f"spread {hp}x{wp} {window}: max fp32 error {ulps.max():.2f} ulp; mean rel err {np.abs(res / mean64 - 1).max():.2e}")
    assert ulps.max() <= 2 and np.array_equal(f32 == 0, s64 == 0)
    near = np.abs(v64 - np.rint(v64)) <= 1e-6                              # within 1e-6 of a rounding boundary: either side is right
    assert near.mean() <= 1e-3, "the reference alone must leave at most 0.1 % of the pixels undecided (choose another seed)"
    assert np.array_equal(u8[~near], np.floor(v64).astype(np.uint8)[~near])
    assert (u8 == 255).any() and (u8 == 0).any()                           # the saturated and the agreed pixels are there
    assert np.all(np.abs(res - mean64) <= 1e-6 * mean64)
    # either output alone: the same bits
    lib = pkg._native.lib()
    src, top, left, h, w = torch.from_numpy(m2).to(DEV), *window
    need = lib.vcg_spread_workspace(n, h, w)
    for want_f32 in (True, False):
        out, res2, ws = Out(n * h * w * (4 if want_f32 else 1)), Out(n * 4), Out(need)
        pkg._native.check(lib.vcg_spread_display_hw(_p(src), COUNT, GAIN, out.ptr() if want_f32 else None, None if want_f32 else out.ptr(),
                                                    res2.ptr(), n, hp, wp, top, left, h, w, ws.ptr(), need, None), "vcg_spread_display_hw")
        got = out.get(torch.float32 if want_f32 else torch.uint8, (n, h, w))
        assert np.array_equal(got, f32 if want_f32 else u8) and np.array_equal(_bits(res2.get(torch.float32, (n,))), _bits(res))
    # the wrapper
    ops = pkg.ops
    M2 = ops.logical_of(torch.from_numpy(np.where(np.isnan(m2), 0, m2).astype(np.float32)).to(DEV), 3)
    (a, b), r = ops.spread_display_hw(M2, COUNT, window, GAIN, uint8="both")
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(f32)) and np.array_equal(b.cpu().numpy(), u8)
    assert np.array_equal(_bits(r.cpu().numpy()), _bits(res))
    assert torch.equal(ops.spread_display_hw(M2, COUNT, window, GAIN)[0], a) and torch.equal(ops.spread_display_hw(M2, COUNT, window, GAIN, uint8=True)[0], b)


def test_the_interior_window_does_not_fit_the_small_buffer(pkg):
    """(3, 5, 20, 37) is 37 wide: inside 48 x 64, not inside 32 x 32 — there the call is refused, not clipped."""
    lib = pkg._native.lib()
    m2 = torch.zeros((1, 32, 32, 4), device=DEV)
    out, res, ws = Out(20 * 37 * 4), Out(4), Out(256)
    assert lib.vcg_spread_display_hw(_p(m2), COUNT, GAIN, out.ptr(), None, res.ptr(), 1, 32, 32, 3, 5, 20, 37, ws.ptr(), 256, None) != 0
    assert b"leaves" in lib.vcg_last_error()
    assert np.isnan(out.get(torch.float32, (20, 37))).all()


def test_spread_reads_nothing_outside_the_window_and_ignores_the_batch(pkg):
    window = (3, 5, 20, 37)
    top, left, h, w = window
    m2 = _spread_m2(3, 48, 64)
    clean = _spread(pkg, m2, window)
    dirty_in = m2.copy()
    mask = np.ones((48, 64), bool)
    mask[top:top + h, left:left + w] = False
    dirty_in[:, mask] = np.nan
    dirty_in[0, mask] = np.inf
    dirty = _spread(pkg, dirty_in, window)
    for a, b in zip(clean, dirty):                                         # fp32 map, uint8 map, per-image mean
        assert np.isfinite(b.astype(np.float64)).all() and a.tobytes() == b.tobytes()
    alone = _spread(pkg, np.ascontiguousarray(m2[1:2]), window)
    assert np.array_equal(_bits(alone[2]), _bits(clean[2][1:2])), "an image's mean must not depend on the batch it is in"
    assert np.array_equal(_bits(alone[0]), _bits(clean[0][1:2])) and np.array_equal(alone[1], clean[1][1:2])
    again = _spread(pkg, m2, window)
    assert all(np.array_equal(a, b) for a, b in zip(clean, again))
