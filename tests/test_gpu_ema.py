"""Averaged generator weights (EMA): vcg_ema_update and vcg_swap through the C ABI (csrc/ema.hip), FusedAdam(ema_decay=...) against a
twin without it, the models' ema_scope, and the checkpoint round trip.

A. vcg_ema_update against float64, element by element.  exact = e + w (p - e) in double from the fp32 inputs and the fp32 w the C
   ABI receives.  Bound per element: 2^-23 (|p| + |e|) + 2^-149 — one rounding of p - e (<= 2^-24 (|p| + |e|), times w <= 1), one
   rounding of the FMA's result (<= 2^-24 max(|p|, |e|): the result lies between e and p), and the subnormal floor.
B. vcg_swap on arbitrary bit patterns (NaN payloads included).
C. FusedAdam(ema_decay=0.999): parameters and moments bit for bit those of a twin without the average; the average against the
   one-step float64 formula with the scheduled decay, within A's bound; a skipped step; ema_state / load_ema_state.
D. Autoencoder (batch 2, 32 x 32) and CycleVAEGAN (batch 2, 256 x 256: the discriminators' 16 x 16 head admits no other size):
   ema_decay=0.0 is the step as it was, 0.999 does not perturb training, ema_scope evaluates exactly the averaged weights and puts
   the raw ones back, packs included.
E. utils.save_checkpoint / load_checkpoint / load_model_weights with the `vcg_ema` key."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EMA_THREADS, EMA_MAX_BLOCKS = 256, 2048                 # csrc/ema.hip: lanes per workgroup, cap of the grid
FULL_PASS = EMA_THREADS * EMA_MAX_BLOCKS * 4            # floats one pass of the grid covers
SIZES = [1, 2, 3, 4, 5, 7, 1023, FULL_PASS + 4 + 1]     # the last: one float4 of a second pass and a one-element tail
GUARD = 64
DECAYS = [0.0, 2.0 / 11.0, 0.999, 0.9999]
WEIGHTS = [1.0 - d for d in DECAYS] + [0.0]             # w = 1 (d = 0): the copy; w = 0: nothing happens
KINDS = ["randn", "tiers", "subnormal", "same"]
LR, B1, B2 = 2e-4, 0.5, 0.999
REFERENCE_KEYS = {"epoch", "model_state_dict", "optimizer_states", "loss", "args"}


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(x):
    """the scalar as the C ABI receives it"""
    return float(np.float32(x))


def contents(n, kind, seed):
    """test_gpu_grad_clip.contents' patterns, with a seed: p and e are drawn apart"""
    rng = np.random.default_rng(seed * 7919 + n % 997)
    if kind == "randn":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "subnormal":
        bits = rng.integers(1, 1 << 23, n, dtype=np.int64).astype(np.uint32) | (rng.integers(0, 2, n, dtype=np.int64).astype(np.uint32) << 31)
        return bits.view(np.float32)
    if kind == "tiers":           # the magnitude changes by up to 2^60 every 64 elements
        t = rng.choice([0, 9, 19, 30, 60], size=(n + 63) // 64)
        return (rng.standard_normal(n) * 2.0 ** -np.repeat(t, 64)[:n].astype(np.float64)).astype(np.float32)
    raise KeyError(kind)


def pair(n, kind):
    if kind == "same":
        p = contents(n, "randn", 1)
        return p, p.copy()
    return contents(n, kind, 1), contents(n, kind, 2)


class Guarded:
    """n floats on the device followed by GUARD NaNs"""

    def __init__(self, values, device):
        self.n = values.size
        self.buf = torch.full((self.n + GUARD,), float("nan"), dtype=torch.float32, device=device)
        self.t = self.buf[:self.n]
        self.t.copy_(torch.from_numpy(values))
        self.guard0 = self.buf[self.n:].view(torch.int32).clone()

    def bits(self, what):
        torch.cuda.synchronize()
        assert torch.equal(self.buf[self.n:].view(torch.int32), self.guard0), f"{what}: the guard region behind the buffer was written"
        assert torch.isnan(self.buf[self.n:]).all().item()
        return self.t.cpu().numpy().view(np.int32).copy()


def bound_of(p, e):
    return 2.0 ** -23 * (np.abs(p.astype(np.float64)) + np.abs(e.astype(np.float64))) + 2.0 ** -149


def ema_exact(p, e, w):
    p64, e64 = p.astype(np.float64), e.astype(np.float64)
    return e64 + f32(w) * (p64 - e64)


def check_within_bound(got, p, e, w, what):
    err = np.abs(got.astype(np.float64) - ema_exact(p, e, w))
    ratio = err / bound_of(p, e)
    i = int(np.argmax(ratio))
    print(f"{what}: worst error {ratio[i]:.3f} x the bound (element {i})")
    assert ratio[i] <= 1.0, f"{what}: element {i}: got {got[i]!r}, exact {ema_exact(p, e, w)[i]!r}, p {p[i]!r}, e {e[i]!r}: {ratio[i]:.3f} x the bound"
    return float(ratio[i])


def run_ema(pkg, device, p, e, w, skip=None):
    """one call on fresh guarded copies -> (bits of e afterwards, bits of p afterwards)"""
    pg, eg = Guarded(p, device), Guarded(e, device)
    pkg._native.check(pkg._native.lib().vcg_ema_update(P(eg.t), P(pg.t), e.size, w, P(skip), _st()), "vcg_ema_update")
    return eg.bits("e"), pg.bits("p")


# ====================================================================================================================== A
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_against_float64(n, pkg, device):
    assert [f32(w) for w in WEIGHTS][0] == 1.0 and f32(WEIGHTS[-1]) == 0.0
    for kind in KINDS:
        p, e = pair(n, kind)
        pbits, ebits = p.view(np.int32), e.view(np.int32)
        for w in WEIGHTS:
            what = f"vcg_ema_update n={n} {kind} w={f32(w)!r}"
            got_bits, p_after = run_ema(pkg, device, p, e, w)
            got = got_bits.view(np.float32)
            assert np.array_equal(p_after, pbits), f"{what}: p was written"
            check_within_bound(got, p, e, w, what)
            if f32(w) == 1.0:
                assert np.array_equal(got_bits, pbits), f"{what}: not an exact copy"
            if f32(w) == 0.0:
                assert np.array_equal(got_bits, ebits), f"{what}: e changed"
            if kind == "same":
                assert np.array_equal(got_bits, pbits), f"{what}: e == p must stay p"
            again, _ = run_ema(pkg, device, p, e, w)
            assert np.array_equal(again, got_bits), f"{what}: two calls, two results"
    # an ordinary weight moves the elements (all but a pair that happens to be equal): a kernel that skipped some would show above
    p, e = pair(n, "randn")
    moved, _ = run_ema(pkg, device, p, e, 0.5)
    assert (moved != e.view(np.int32)).sum() >= n - 1


@pytest.mark.parametrize("n", [5, 1023, FULL_PASS + 4 + 1])
def test_ema_update_obeys_the_skip_flag(n, pkg, device):
    p, e = pair(n, "randn")
    w = 1.0 - 0.999
    plain, _ = run_ema(pkg, device, p, e, w)
    for wt in (w, 1.0):
        skipped, p_after = run_ema(pkg, device, p, e, wt, torch.tensor([0.0, 0.0, 1.0, 0.0], device=device))
        assert np.array_equal(skipped, e.view(np.int32)), f"n={n} w={wt}: a skipped update wrote"
        assert np.array_equal(p_after, p.view(np.int32))
    clear, _ = run_ema(pkg, device, p, e, w, torch.tensor([3.0, 0.5, 0.0, 0.0], device=device))
    assert np.array_equal(clear, plain), f"n={n}: a clear flag changed the result"
    assert not np.array_equal(plain, e.view(np.int32))


def test_ema_update_refuses_bad_arguments(pkg, device):
    lib = pkg._native.lib()
    p, e = pair(1000, "randn")
    pg, eg = Guarded(p, device), Guarded(e, device)

    def bad(match, *args):
        assert lib.vcg_ema_update(*args) != 0, match
        assert match in lib.vcg_last_error(), (match, lib.vcg_last_error())

    bad(b"null pointer", None, P(pg.t), 1000, 0.5, None, _st())
    bad(b"null pointer", P(eg.t), None, 1000, 0.5, None, _st())
    for w in (1.5, -0.5, float("nan"), float("inf")):
        bad(b"[0, 1]", P(eg.t), P(pg.t), 1000, w, None, _st())
    bad(b"aligned", P(eg.t[1:]), P(pg.t), 996, 0.5, None, _st())
    bad(b"aligned", P(eg.t), P(pg.t[2:]), 996, 0.5, None, _st())
    assert np.array_equal(eg.bits("e"), e.view(np.int32)) and np.array_equal(pg.bits("p"), p.view(np.int32))      # nothing was launched
    assert lib.vcg_ema_update(P(eg.t), P(pg.t), 0, 0.5, None, _st()) == 0
    assert np.array_equal(eg.bits("e"), e.view(np.int32))


# ====================================================================================================================== B
def _patterns(n, seed):
    """arbitrary words: NaNs with payloads, infinities, subnormals and zeros of both signs among them"""
    bits = np.random.default_rng(seed + n % 991).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], dtype=np.uint32)
    k = min(n, special.size)
    bits[-k:] = np.roll(special, seed // 10)[:k]             # the tail elements are among them; the two buffers get them in another order
    return bits.view(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bits(n, pkg, device):
    lib = pkg._native.lib()
    a, b = _patterns(n, 10), _patterns(n, 20)
    abits, bbits = a.view(np.int32), b.view(np.int32)
    assert not np.array_equal(abits, bbits)
    ag, bg = Guarded(a, device), Guarded(b, device)
    pkg._native.check(lib.vcg_swap(P(ag.t), P(bg.t), n, _st()), "vcg_swap")
    assert np.array_equal(ag.bits("a"), bbits) and np.array_equal(bg.bits("b"), abits), f"n={n}: one swap"
    pkg._native.check(lib.vcg_swap(P(ag.t), P(bg.t), n, _st()), "vcg_swap")
    assert np.array_equal(ag.bits("a"), abits) and np.array_equal(bg.bits("b"), bbits), f"n={n}: two swaps are not the identity"


def test_swap_refuses_bad_arguments(pkg, device):
    lib = pkg._native.lib()
    a = _patterns(64, 30)
    g = Guarded(a, device)
    other = Guarded(a, device)

    def bad(match, *args):
        assert lib.vcg_swap(*args) != 0, match
        assert match in lib.vcg_last_error(), (match, lib.vcg_last_error())

    bad(b"null pointer", None, P(g.t), 8, _st())
    bad(b"null pointer", P(g.t), None, 8, _st())
    bad(b"overlap", P(g.t), P(g.t[4:]), 8, _st())           # [0, 8) and [4, 12)
    bad(b"overlap", P(g.t[4:]), P(g.t), 8, _st())
    bad(b"overlap", P(g.t), P(g.t), 8, _st())
    bad(b"aligned", P(g.t), P(other.t[1:]), 8, _st())
    assert np.array_equal(g.bits("a"), a.view(np.int32)) and np.array_equal(other.bits("b"), a.view(np.int32))
    pkg._native.check(lib.vcg_swap(P(g.t), P(g.t[8:]), 8, _st()), "vcg_swap")                 # adjacent ranges do not overlap
    assert np.array_equal(g.bits("a")[:16], np.concatenate([a.view(np.int32)[8:16], a.view(np.int32)[:8]]))
    assert lib.vcg_swap(P(g.t), P(g.t), 0, _st()) == 0


# ====================================================================================================================== C
SHAPES = [(5, 3, 3, 3), (5,), (7, 5, 1, 1)]                  # 135 + 5 + 35 parameters: none a multiple of 4 (5 padding elements)
DECAY = 0.999


def _fused(pkg, device, init, **kw):
    params = [torch.nn.Parameter(t.clone().to(device)) for t in init]
    return params, pkg.optim.FusedAdam(params, lr=LR, betas=(B1, B2), **kw)


def _init_and_grads(steps=5):
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen) * 0.1 for s in SHAPES]
    return init, [[torch.randn(s, generator=gen) for s in SHAPES] for _ in range(steps)]


def _feed(opt, params, grads, device):
    opt.zero_grad()
    for p, g in zip(params, grads):
        p.grad.copy_(g.to(device))


def _opt_bits(opt, names=("flat_param", "exp_avg", "exp_avg_sq")):
    torch.cuda.synchronize()
    return {n: getattr(opt, n).view(torch.int32).clone() for n in names}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs in {(a[k] != b[k]).sum().item()} of {a[k].numel()} elements"


def test_fused_adam_keeps_the_average_and_trains_as_its_twin(pkg, device):
    at = pkg.optim.ema_decay_at
    init, grads = _init_and_grads()
    pa, a = _fused(pkg, device, init, ema_decay=DECAY)
    pb, b = _fused(pkg, device, init)
    assert b.flat_ema is None and b.ema_decay is None and a.ema_decay == DECAY and a.ema_updates == 0
    assert a.flat_ema.numel() == a.total == 180 and a.flat_ema.abs().max().item() == 0.0
    used = torch.zeros(a.total, dtype=torch.bool)
    for p, o in zip(a.params, a.offsets):
        used[o:o + p.numel()] = True
    assert (~used).sum().item() == 5
    for step, g in enumerate(grads):
        prev = a.flat_ema.cpu().numpy().copy()
        _feed(a, pa, g, device)
        _feed(b, pb, g, device)
        a.step()
        b.step()
        _same(_opt_bits(a), _opt_bits(b), f"step {step}: with and without the average")
        assert a.ema_updates == step + 1
        cur, ema = a.flat_param.cpu().numpy(), a.flat_ema.cpu().numpy()
        if step == 0:
            assert np.array_equal(ema.view(np.int32), cur.view(np.int32)), "the first update must copy the parameters"
        else:
            d = at(DECAY, step)
            assert d == min(DECAY, (1.0 + step) / (10.0 + step))
            check_within_bound(ema, cur, prev, 1.0 - d, f"FusedAdam average after step {step} (decay {d:.4f})")
            assert not np.array_equal(ema.view(np.int32), cur.view(np.int32)) and not np.array_equal(ema.view(np.int32), prev.view(np.int32))
        assert np.abs(ema[~used.numpy()]).max() == 0.0 and np.abs(cur[~used.numpy()]).max() == 0.0, "the padding moved"
    # torch.optim.Adam's layout does not know about the average
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) and [set(g) for g in sa["param_groups"]] == [set(g) for g in sb["param_groups"]]
    assert all(set(sa["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} for i in sa["state"])
    assert "ema_decay" not in a.param_groups[0] and "ema_decay" not in a.defaults
    # ema_state -> load_ema_state into a fresh optimizer
    state = a.ema_state()
    assert state["decay"] == DECAY and state["updates"] == 5 and [tuple(t.shape) for t in state["tensors"]] == SHAPES
    _, fresh = _fused(pkg, device, init, ema_decay=DECAY)
    fresh.load_ema_state({k: ([t.cpu() for t in v] if k == "tensors" else v) for k, v in state.items()})
    assert fresh.ema_updates == 5
    _same(_opt_bits(fresh, ("flat_ema",)), _opt_bits(a, ("flat_ema",)), "load_ema_state")
    with pytest.raises(ValueError, match="parameter"):
        fresh.load_ema_state(dict(state, tensors=state["tensors"][:2]))
    with pytest.raises(ValueError, match="shape"):
        fresh.load_ema_state(dict(state, tensors=[state["tensors"][0], state["tensors"][2], state["tensors"][1]]))
    with pytest.raises(RuntimeError, match="no average"):
        b.ema_state()
    for bad in (0.0, 1.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ema_decay"):
            _fused(pkg, device, init, ema_decay=bad)


def test_swap_ema_exchanges_and_restores(pkg, device):
    init, grads = _init_and_grads(2)
    pa, a = _fused(pkg, device, init, ema_decay=DECAY)
    for g in grads:
        _feed(a, pa, g, device)
        a.step()
    before = _opt_bits(a, ("flat_param", "flat_ema"))
    epoch, global_epoch = a._epoch[0], pkg.ops.PARAM_EPOCH[0]
    a.swap_ema()
    mid = _opt_bits(a, ("flat_param", "flat_ema"))
    assert torch.equal(mid["flat_param"], before["flat_ema"]) and torch.equal(mid["flat_ema"], before["flat_param"])
    assert torch.equal(pa[0].detach().view(torch.int32).flatten(), before["flat_ema"][:135])       # the parameters ARE the buffer
    assert a._epoch[0] > epoch and pkg.ops.PARAM_EPOCH[0] > global_epoch and a.ema_swapped
    with pytest.raises(RuntimeError, match="swapped in"):
        a.step()
    with pytest.raises(RuntimeError, match="swapped in"):
        a.ema_state()
    a.swap_ema()
    _same(_opt_bits(a, ("flat_param", "flat_ema")), before, "two swaps")
    assert not a.ema_swapped and a.ema_updates == 2
    # an average no update has reached is the parameters
    pz, z = _fused(pkg, device, init, ema_decay=DECAY)
    assert all(torch.equal(t, p.detach()) for t, p in zip(z.ema_state()["tensors"], pz)) and z.ema_updates == 0


def test_a_skipped_step_leaves_the_average_alone(pkg, device):
    init, grads = _init_and_grads(4)
    pa, a = _fused(pkg, device, init, ema_decay=DECAY, max_grad_norm=5.0)
    names = ("flat_param", "exp_avg", "exp_avg_sq", "flat_ema")
    for g in grads[:2]:
        _feed(a, pa, g, device)
        a.step()
    kept = _opt_bits(a, names)
    bad = [g.clone() for g in grads[2]]
    bad[2].view(-1)[34] = float("nan")                        # the last element of the last parameter
    _feed(a, pa, bad, device)
    a.step()
    assert a.clip_state[2].item() == 1.0
    _same(_opt_bits(a, names), kept, "a step on a NaN gradient")
    assert a.ema_updates == 3                                 # the host does not see the skip (FusedAdam's docstring)
    _feed(a, pa, grads[3], device)
    a.step()
    after = _opt_bits(a, names)
    assert all(not torch.equal(after[k], kept[k]) for k in names) and a.clip_state[2].item() == 0.0


# ====================================================================================================================== D
ARCHS = {"autoencoder": (32, 2), "cyclevaegan": (256, 2)}      # image size, batch


def _make(pkg, device, arch, **opt_kw):
    torch.manual_seed(5)
    model = pkg.Networks.Autoencoder() if arch == "autoencoder" else pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False)
    model = model.to(device).train()
    model.configure_optimizers(lr=LR, **opt_kw)
    model.configure_loss()
    pkg.ops.manual_seed(11)                                    # the eps stream of the model's first step
    return model


def _batch(pkg, device, arch, step):
    S, B = ARCHS[arch]
    x, y = pkg.synth.batch(B, S, 20261019, step=step)
    xb = torch.from_numpy(x).to(device)
    return {"x": xb, "y": xb if arch == "autoencoder" else torch.from_numpy(y).to(device)}


def _opts(model):
    return {sfx: getattr(model, "optimizer" + sfx) for sfx in ("", "_G", "_D") if getattr(model, "optimizer" + sfx, None) is not None}


def _state(model):
    """parameters, both moment buffers and (where kept) the average of every optimizer, as bits"""
    torch.cuda.synchronize()
    return {(sfx, name): getattr(o, name).view(torch.int32).clone() for sfx, o in _opts(model).items()
            for name in ("flat_param", "exp_avg", "exp_avg_sq", "flat_ema") if getattr(o, name, None) is not None}


def _without_ema(state):
    return {k: v for k, v in state.items() if k[1] != "flat_ema"}


def _steps(pkg, device, model, arch, steps):
    out = []
    for step in steps:
        pkg.ops.manual_seed(1000 + step)
        m = model.training_step(_batch(pkg, device, arch, step))
        out.append((m, _state(model)))
    return out


def _validate(pkg, model, batch):
    model.eval()
    pkg.ops.manual_seed(77)                                    # the same position of the eps stream for everyone
    v = model.validation_step(batch)
    model.train()
    torch.cuda.synchronize()
    images = {k: v.pop(k).contiguous().view(torch.int32).clone() for k in ("Gx", "Fy") if k in v}
    return v, images


@pytest.mark.parametrize("arch", list(ARCHS))
def test_off_is_the_step_as_it_was(arch, pkg, device):
    plain = _make(pkg, device, arch)
    a = _steps(pkg, device, plain, arch, [0, 1])
    off = _make(pkg, device, arch, ema_decay=0.0)
    b = _steps(pkg, device, off, arch, [0, 1])
    assert off.ema_enabled is False and all(o.flat_ema is None and o.ema_decay is None for o in _opts(off).values())
    for step, ((m0, s0), (m1, s1)) in enumerate(zip(a, b)):
        assert list(m0) == list(m1) and m0 == m1, (step, m0, m1)
        _same(s0, s1, f"{arch} step {step}, ema_decay=0.0")
    with off.ema_scope():                                      # a no-op: nothing is swapped, nothing repacked
        pass
    _same(_state(off), b[-1][1], f"{arch}: ema_scope of a model without an average")


@pytest.mark.parametrize("arch", list(ARCHS))
def test_average_does_not_perturb_training_and_the_scope_evaluates_it(arch, pkg, device):
    plain = _make(pkg, device, arch)
    a = _steps(pkg, device, plain, arch, [0, 1, 2])
    model = _make(pkg, device, arch, ema_decay=DECAY)
    b = _steps(pkg, device, model, arch, [0, 1])
    for step in range(2):
        assert list(a[step][0]) == list(b[step][0]) and a[step][0] == b[step][0], (step, a[step][0], b[step][0])
        _same(a[step][1], _without_ema(b[step][1]), f"{arch} step {step}: with and without the average")
    opts = _opts(model)
    tracked = opts["_G" if arch == "cyclevaegan" else ""]
    assert model.ema_enabled and tracked.ema_updates == 2
    if arch == "cyclevaegan":
        assert opts["_D"].flat_ema is None and opts["_D"].ema_decay is None        # discriminators are not averaged
    raw = {k: v.detach().clone() for k, v in model.state_dict().items()}
    avg = model.ema_state_dict()
    names = {id(p): n for n, p in model.named_parameters()}
    assert list(avg) == [names[id(p)] for p in tracked.params] and set(avg) <= set(raw)
    assert all(avg[k].shape == raw[k].shape for k in avg) and any(not torch.equal(avg[k], raw[k]) for k in avg)
    if arch == "cyclevaegan":
        assert not any(k.startswith(("DX.", "DY.")) for k in avg) and any(k.startswith("G.") for k in avg) and any(k.startswith("F.") for k in avg)
    before = _state(model)

    # a third model that simply HOLDS the averaged weights
    third = _make(pkg, device, arch)
    third.load_state_dict(dict(raw, **avg))
    pkg.ops.PARAM_EPOCH[0] += 1
    batch = _batch(pkg, device, arch, 7)
    want, want_images = _validate(pkg, third, batch)
    raw_metrics, _ = _validate(pkg, model, batch)
    with model.ema_scope() as scoped:
        assert scoped is model
        got, got_images = _validate(pkg, model, batch)
        inside = {k: v.detach().clone() for k, v in model.state_dict().items()}
        with pytest.raises(RuntimeError, match="nest"):
            with model.ema_scope():
                pass
    assert list(got) == list(want) and got == want, f"{arch}: validation inside ema_scope: {got} vs {want}"
    assert got_images.keys() == want_images.keys() and all(torch.equal(got_images[k], want_images[k]) for k in got_images)
    assert got != raw_metrics                                  # ... and it is not what the raw weights give
    assert all(torch.equal(inside[k], avg[k] if k in avg else raw[k]) for k in raw)
    _same(_state(model), before, f"{arch}: after ema_scope")
    again, _ = _validate(pkg, model, batch)
    assert again == raw_metrics                                # the raw weights' packs are back too

    # training inside the scope is refused, and the failed block still puts the raw weights back
    with pytest.raises(RuntimeError, match="ema_scope"):
        with model.ema_scope():
            model.training_step(_batch(pkg, device, arch, 2))
    _same(_state(model), before, f"{arch}: after a block that raised inside ema_scope")
    assert tracked.ema_swapped is False and tracked.ema_updates == 2

    c = _steps(pkg, device, model, arch, [2])
    assert list(a[2][0]) == list(c[0][0]) and a[2][0] == c[0][0], (a[2][0], c[0][0])
    _same(a[2][1], _without_ema(c[0][1]), f"{arch}: the step after ema_scope")
    assert tracked.ema_updates == 3


# ====================================================================================================================== E
def _args():
    return argparse.Namespace(architecture="autoencoder", lr=LR, ema_decay=DECAY)


def test_checkpoint_round_trip(pkg, device, tmp_path, capsys):
    utils, arch = pkg.utils, "autoencoder"
    model = _make(pkg, device, arch, ema_decay=DECAY)
    _steps(pkg, device, model, arch, [0, 1])
    path = tmp_path / "with_average.pth"
    utils.save_checkpoint(model, 3, 0.5, _args(), str(path), best_test_loss=0.25)
    ck = torch.load(str(path), map_location="cpu", weights_only=False)
    assert set(ck) - REFERENCE_KEYS == {"vcg_eps_rng", "vcg_best_test_loss", "vcg_ema"}
    assert set(ck["vcg_ema"]) == {"decay", "updates", "state_dict"} and ck["vcg_ema"]["decay"] == DECAY and ck["vcg_ema"]["updates"] == 2
    assert list(ck["vcg_ema"]["state_dict"]) == list(ck["model_state_dict"])           # the autoencoder tracks every parameter
    assert all(not t.is_cuda for t in ck["vcg_ema"]["state_dict"].values())
    raw_now = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    assert all(torch.equal(ck["model_state_dict"][k], raw_now[k]) for k in raw_now)    # the file's weights are the raw ones
    assert any(not torch.equal(ck["vcg_ema"]["state_dict"][k], raw_now[k]) for k in raw_now)
    (m_want, s_want), = _steps(pkg, device, model, arch, [2])                          # the uninterrupted run

    resumed = _make(pkg, device, arch, ema_decay=DECAY)
    assert utils.load_checkpoint(resumed, str(path), device) == (3, 0.5)
    assert resumed.optimizer.ema_updates == 2
    (m_got, s_got), = _steps(pkg, device, resumed, arch, [2])
    assert m_got == m_want
    _same(s_got, s_want, "the step after a resume")
    assert ("", "flat_ema") in s_got and resumed.optimizer.ema_updates == model.optimizer.ema_updates == 3

    # the averaged weights for inference
    fresh = pkg.Networks.Autoencoder().to(device)
    rest = utils.load_model_weights(fresh, str(path), ema=True)
    assert rest["epoch"] == 3 and "vcg_ema" not in rest
    got = fresh.state_dict()
    assert all(torch.equal(got[k].cpu(), ck["vcg_ema"]["state_dict"][k]) for k in got)
    utils.load_model_weights(fresh, str(path))
    assert all(torch.equal(fresh.state_dict()[k].cpu(), raw_now[k]) for k in raw_now)

    # without the feature: no key; such a file starts the average from its weights; a file with the key loads into a plain model
    off = _make(pkg, device, arch)
    _steps(pkg, device, off, arch, [0])
    plain_path = tmp_path / "plain.pth"
    utils.save_checkpoint(off, 0, 0.5, _args(), str(plain_path))
    plain_ck = torch.load(str(plain_path), map_location="cpu", weights_only=False)
    assert set(plain_ck) - REFERENCE_KEYS == {"vcg_eps_rng"}
    with pytest.raises(KeyError, match="plain.pth"):
        utils.load_model_weights(fresh, str(plain_path), ema=True)
    capsys.readouterr()
    lazy = _make(pkg, device, arch, ema_decay=DECAY)
    utils.load_checkpoint(lazy, str(plain_path), device)
    assert "no averaged weights" in capsys.readouterr().out and lazy.optimizer.ema_updates == 0
    assert all(torch.equal(t.cpu(), plain_ck["model_state_dict"][k]) for k, t in lazy.ema_state_dict().items())
    utils.load_checkpoint(off, str(path), device)              # `vcg_ema` is ignored by a model that keeps no average
    assert off.ema_enabled is False and all(torch.equal(off.state_dict()[k].cpu(), raw_now[k]) for k in raw_now)
