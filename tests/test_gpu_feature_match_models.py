"""GPU: the discriminator feature-matching term (configure_loss(lambda_fm=..., fm_mode=...)) in the GAN models — it leaves the
discriminator update alone, the generator gradient it adds is the term's (against a stand-in composed from other ops), loss_fm is
the float64 restatement (tests/test_feature_match_host.py) on what Discriminator.features returned, two direction streams give
the bits of one, validation reports it and touches nothing, it runs on the patch head, and two ranks exchange the sum of what their
shards give alone.

256 x 256 is the smallest image the discriminator head accepts (272 x 256 gives the patch head two logits); batch 1, batch 2 where
the element-wise mode pairs images; latent_dim 8; one step each.  Weights are the constructors' own draws under a fixed torch
seed (a twin is a second instance loaded with the first one's state_dict); eps comes from the on-device stream, reseeded before
every step that is compared.  The steps that several tests look at run once (`runs`)."""
import shutil
import time

import pytest
import torch

from test_feature_match_host import fm_reference
from test_gpu_gan_objective_models import EPS_SEED, instances, ready, step

pytestmark = pytest.mark.gpu

LAMBDA_FM = 10.0
REL = 2.0 ** -22                          # loss_fm against the float64 restatement / the stand-in
GRAD_BOUND = 1e-4                         # the project's per-op bound (README, parity row), per parameter, of its gradient's maximum
CASES = [("aegan", "pair", 2), ("cyclevaegan", "mean", 1)]
NOT_COMPARED = ("G_loss", "total_loss", "loss_fm")


def batch_of(pkg, device, n, height=256):
    x = pkg.ops.rand_uniform((n, 3, height, 256), device, seed=91, offset=0)
    y = pkg.ops.rand_uniform((n, 3, height, 256), device, seed=91, offset=1 << 22)
    return {"x": x, "y": y}


def discriminators(model):
    return [getattr(model, n) for n in model._discriminators]


def record_features(model):
    """Wraps every discriminator's `features` -> {discriminator name: [(activations, logits) of every call, in order]}."""
    seen = {}
    for name in model._discriminators:
        D = getattr(model, name)
        seen[name] = []

        def wrapped(x, inner=D.features, calls=seen[name]):
            acts, logits = inner(x)
            calls.append(([a.detach().clone() for a in acts], logits.detach().clone()))
            return acts, logits
        D.features = wrapped
    return seen


def restated(seen, mode):
    """The term in float64 on the recorded calls: every discriminator saw its fakes first, then its real images; the cycle models
    add the two discriminators' terms."""
    total = 0.0
    for calls in seen.values():
        assert len(calls) == 2 and len(calls[0][0]) == 4, [len(c[0]) for c in calls]
        total += fm_reference(calls[0][0], calls[1][0], mode).item()
    return total


def snapshot(model):
    torch.cuda.synchronize()
    return {f"{o}.{buf}": getattr(getattr(model, o), buf).detach().clone() for o in ("optimizer_G", "optimizer_D")
            for buf in ("flat_param", "flat_grad")}


_RUNS = {}


def runs(pkg, device, arch, mode, n):
    """One training step of twins from one seed with lambda_fm 0 and 10 -> {"off" / "on": (metrics, snapshot), "seen": the
    recorded features of the run with the term, "offsets": optimizer_G's (offset, numel) per parameter}."""
    key = (arch, mode, n)
    if key not in _RUNS:
        off, on = instances(pkg, arch, 2)
        off, on = ready(off, device), ready(on, device, lambda_fm=LAMBDA_FM, fm_mode=mode)
        assert off.fm_term is None and on.fm_term is not None
        seen = record_features(on)
        batch = batch_of(pkg, device, n)
        out = {"seen": seen, "offsets": [(o, p.numel()) for p, o in zip(on.optimizer_G.params, on.optimizer_G.offsets)]}
        for name, model in (("off", off), ("on", on)):
            m = step(pkg, model, batch)
            out[name] = (m, snapshot(model))
        _RUNS[key] = out
    return _RUNS[key]


def bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------ 1. the discriminator update is untouched
@pytest.mark.parametrize("arch,mode,n", CASES)
def test_the_discriminator_update_is_untouched(arch, mode, n, pkg, device):
    r = runs(pkg, device, arch, mode, n)
    (m_off, s_off), (m_on, s_on) = r["off"], r["on"]
    assert "loss_fm" not in m_off and list(m_on) == list(m_off) + ["loss_fm"], (list(m_off), list(m_on))
    assert m_on["loss_fm"] > 0.0
    assert torch.equal(bits(s_on["optimizer_D.flat_param"]), bits(s_off["optimizer_D.flat_param"]))
    assert torch.equal(bits(s_on["optimizer_D.flat_grad"]), bits(s_off["optimizer_D.flat_grad"]))
    assert not torch.equal(bits(s_on["optimizer_G.flat_param"]), bits(s_off["optimizer_G.flat_param"]))
    for k, v in m_off.items():
        if k not in NOT_COMPARED:
            assert m_on[k] == v, f"{k}: {m_on[k]!r} with the term, {v!r} without"
    assert m_on["G_loss"] != m_off["G_loss"]
    # G_loss carries lambda_fm loss_fm: two fp32 weighted sums of the same non-negative terms (at most 7 products and 6 additions
    # each, every partial sum below the total), one more term in one of them
    assert abs(m_on["G_loss"] - m_off["G_loss"] - LAMBDA_FM * m_on["loss_fm"]) <= 16 * 2.0 ** -24 * (abs(m_on["G_loss"]) + abs(m_off["G_loss"]))


# ------------------------------------------------------------------ 2. the generator gradient is the term's
def standin(pkg, mode):
    ops = pkg.ops

    def pair(fakes, reals, mode_):
        assert mode_ == "pair"
        terms = [ops.l1_loss(f, r.detach()) for f, r in zip(fakes, reals)]
        return ops.weighted_sum(terms, [1.0 / len(terms)] * len(terms))

    def mean(fakes, reals, mode_):
        assert mode_ == "mean"
        terms = [(f.mean(dim=(0, 2, 3)) - r.detach().mean(dim=(0, 2, 3))).abs().mean() for f, r in zip(fakes, reals)]
        return sum(terms) / len(terms)

    return {"pair": pair, "mean": mean}[mode]


@pytest.mark.parametrize("arch,mode,n", CASES)
def test_the_generator_gradient_is_the_terms(arch, mode, n, pkg, device, monkeypatch):
    r = runs(pkg, device, arch, mode, n)
    m_on, s_on = r["on"]
    calls = []
    composed = standin(pkg, mode)
    monkeypatch.setattr(pkg.ops, "feature_matching", lambda *a: calls.append(1) or composed(*a))
    twin = ready(instances(pkg, arch, 1)[0], device, lambda_fm=LAMBDA_FM, fm_mode=mode)
    m = step(pkg, twin, batch_of(pkg, device, n))
    assert len(calls) == len(twin._discriminators), "the model did not look ops.feature_matching up when it called it"
    rel = abs(m["loss_fm"] - m_on["loss_fm"]) / abs(m_on["loss_fm"])
    print(f"{arch} {mode}: loss_fm fused {m_on['loss_fm']!r} composed {m['loss_fm']!r} rel {rel:.3e} (bound {REL:.3e})")
    got, want = s_on["optimizer_G.flat_grad"], snapshot(twin)["optimizer_G.flat_grad"]
    worst, compared = 0.0, 0
    for off, numel in r["offsets"]:
        a, b = got[off:off + numel], want[off:off + numel]
        scale = b.abs().max().item()
        if scale == 0.0:                                 # a bias in front of an InstanceNorm: its gradient is 0 in both runs
            assert a.abs().max().item() == 0.0
            continue
        compared += 1
        worst = max(worst, (a - b).abs().max().item() / scale)
    assert compared >= len(r["offsets"]) // 2
    print(f"{arch} {mode}: optimizer_G.flat_grad fused vs composed, worst parameter {worst:.3e} of its maximum (bound {GRAD_BOUND:g})")
    assert worst <= GRAD_BOUND
    assert rel <= REL
    for k in ("optimizer_D.flat_param", "optimizer_D.flat_grad"):          # and the stand-in's step leaves the discriminators alone too
        assert torch.equal(bits(snapshot(twin)[k]), bits(s_on[k]))


# ------------------------------------------------------------------ 3. loss_fm is the restatement
@pytest.mark.parametrize("arch,mode,n", CASES)
def test_loss_fm_is_the_float64_restatement_on_the_features(arch, mode, n, pkg, device):
    r = runs(pkg, device, arch, mode, n)
    got, want = r["on"][0]["loss_fm"], restated(r["seen"], mode)
    print(f"{arch} {mode}: loss_fm {got!r}, float64 {want!r}, rel {abs(got - want) / abs(want):.3e} (bound {REL:.3e})")
    assert abs(got - want) <= REL * abs(want)


def test_features_is_forward_with_the_activations_kept(pkg, device):
    """One pass: the logits are forward's bits, the activations are the four blocks' outputs."""
    torch.manual_seed(5)
    D = pkg.Networks.Discriminator().to(device).eval()
    x = batch_of(pkg, device, 1)["x"]
    with torch.no_grad():
        logits = D(x)
        acts, again = D.features(x)
    assert torch.equal(bits(again), bits(logits))
    assert [tuple(a.shape) for a in acts] == [(1, 64, 128, 128), (1, 128, 64, 64), (1, 256, 32, 32), (1, 512, 16, 16)]
    assert all(pkg.ops.can_alias(a) for a in acts)


# ------------------------------------------------------------------ 4. two streams against one
def test_two_direction_streams_give_the_bits_of_one(pkg, device):
    assert pkg.ops.DIRECTION_STREAMS and pkg.ops.two_directions(), "the two-stream path is switched off in this environment"
    r = runs(pkg, device, "cyclevaegan", "mean", 1)
    one = ready(instances(pkg, "cyclevaegan", 1)[0], device, lambda_fm=LAMBDA_FM, fm_mode="mean")
    saved = pkg.ops.DIRECTION_STREAMS
    pkg.ops.DIRECTION_STREAMS = False
    try:
        assert not pkg.ops.two_directions()
        m = step(pkg, one, batch_of(pkg, device, 1))
    finally:
        pkg.ops.DIRECTION_STREAMS = saved
    m_two, s_two = r["on"]
    assert m == m_two, (m, m_two)
    s_one = snapshot(one)
    for k in s_one:
        assert torch.equal(bits(s_one[k]), bits(s_two[k])), k


# ------------------------------------------------------------------ 5. validation
@pytest.mark.parametrize("arch,mode,n", CASES)
def test_validation_reports_the_term_and_touches_nothing(arch, mode, n, pkg, device):
    model = ready(instances(pkg, arch, 1)[0], device, lambda_fm=LAMBDA_FM, fm_mode=mode)
    batch = batch_of(pkg, device, n)
    step(pkg, model, batch)                              # gradients and optimizer state exist
    before = snapshot(model)
    grads = [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]
    counts = [list(getattr(model, o).steps) for o in model._opt_names]
    seen = record_features(model)
    model.eval()
    pkg.ops.manual_seed(EPS_SEED)
    m = model.validation_step(dict(batch))
    torch.cuda.synchronize()
    scalars = [k for k, v in m.items() if not isinstance(v, torch.Tensor)]
    assert scalars[-1] == "loss_fm" and list(m)[-1] == "loss_fm", list(m)
    want = restated(seen, mode)
    assert abs(m["loss_fm"] - want) <= REL * abs(want), (m["loss_fm"], want)
    after = snapshot(model)
    for k in before:
        assert torch.equal(bits(after[k]), bits(before[k])), k
    for p, g in zip(model.parameters(), grads):
        assert (p.grad is None) == (g is None) and (g is None or torch.equal(bits(p.grad), bits(g)))
    assert counts == [list(getattr(model, o).steps) for o in model._opt_names]
    model.configure_loss()                               # and without the term validation has the keys it had
    assert "loss_fm" not in model.validation_step(dict(batch))


# ------------------------------------------------------------------ 6. the patch head
def test_vaegan_on_the_patch_head(pkg, device):
    model = ready(instances(pkg, "vaegan", 1)[0], device, lambda_fm=LAMBDA_FM, fm_mode="mean")
    seen = record_features(model)
    m = step(pkg, model, batch_of(pkg, device, 1, height=272))
    assert all(v == v and abs(v) != float("inf") for v in m.values()), m
    (fake_acts, fake_logits), (real_acts, _) = seen["D"]
    assert fake_logits.numel() == pkg.ops.head_output_shape(272, 256)[0] * pkg.ops.head_output_shape(272, 256)[1] == 2
    assert tuple(fake_acts[3].shape) == (1, 512, 17, 16)
    want = restated(seen, "mean")
    print(f"vaegan 272 x 256: loss_fm {m['loss_fm']!r}, float64 {want!r}, rel {abs(m['loss_fm'] - want) / abs(want):.3e}")
    assert list(m)[-1] == "loss_fm" and abs(m["loss_fm"] - want) <= REL * abs(want)


# ------------------------------------------------------------------ 7. two ranks
def test_two_ranks_exchange_the_sum_of_the_shards_alone(pkg, device, tmp_path):
    """AEGAN, element-wise mode, the two-rank set-up of tests/test_gpu_dp_options.py (two ranks share the card at 4 hardware
    queues each): the exchanged gradients are bit for bit the sum of what the two shards give alone, loss_fm is their mean."""
    from test_gpu_dp_architectures import _run_case
    from test_gpu_dp_options import DP_LR, STEPS
    t0 = time.monotonic()

    def reported(i, before, after, m0, m1):
        for rec in after:
            assert list(rec["metrics"])[-1] == "loss_fm" and rec["metrics"]["loss_fm"] > 0.0, rec["metrics"]
        assert m0["loss_fm"] != m1["loss_fm"]            # a rank's own value is not the mean

    try:
        _run_case(pkg, device, tmp_path, "aegan", "fm", DP_LR, STEPS[:1], loss_kw=dict(lambda_fm=LAMBDA_FM, fm_mode="pair"),
                  each_step=reported)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time feature matching under two ranks: {time.monotonic() - t0:.1f} s")
