"""GPU: the data-parallel step (parallel.GradReducer) of the architectures and step options that had never met a second rank,
held to the data-parallel contract itself instead of "equals the big batch":

    after the exchange each rank's flat_grad is, bit for bit, g0 + g1 in fp32, g_r being the flat_grad that ONE process without
    a reducer and without a process group leaves after training_step on shard r alone, started from the state the ranks held
    before the step.

A gloo sum over two ranks is one commutative fp32 addition per element and a step is bit-reproducible across processes and model
instances (test_checkpoint_has_the_reference_format_and_resumes_bit_identically, tests/test_gpu_changing_shapes.py), so the bound
is zero, and it holds where the big batch cannot be the reference at all: the free-bits floor acts on each rank's own batch, the
sliced Wasserstein term draws a plan per rank.

The ranks are test_gpu_dp_options.py's worker (two `spawn` processes on the one card, batch 1 each, gloo with a 60 s group timeout,
4 hardware queues per rank, joined under its limit; a failure terminates both and nothing more is started).  Both write what they
hold before their first step and after every step: metrics, the reducer's log, every buffer of BUFFERS per optimizer and _extras
(spectral norm's u and v, step counters, the average's update count, the sliced Wasserstein term's seed and counter).  The state
before step s is the record after step s - 1.  Parameters and moments are written once, as the optimizers' flat buffers:
state_dict()'s parameters and save_optimizer_states()'s moments are views and clones of exactly these, and the parent loads them
back through load_state_dict / the optimizers' load_state_dict / load_ema_state / load_swd_state (dp._restore).

Per case and step (_check_step): the replicas are bitwise equal; step 0 exchanges every bucket at `start` (it learns the report
counts), every later step launches every bucket of every optimizer from `backward` — the bitwise sum there is the proof that no
slice was reduced while a stream still wrote into it —; flat_grad on both ranks is g0 + g1; every reported metric is 0.5 (m0 + m1)
of the two plain runs to 1e-6 (one fp32 average apart; test_gpu_image_terms.two_ranks_report_the_mean_and_stay_replicas's bound);
the summed gradient stepped in a plain model with grad_scale = 0.5 gives the ranks' parameters, both moments, the average and
clip_state bit for bit.  No property of a model made the plain shard run differ from the rank's: the one place of Networks.py
where a reducer changes the step (_PoolMixin._shown_to) needs pool_size > 0, which stays with test_image_pool_under_two_ranks.

A. the eight architectures of ARCH_CASES, every option off, two steps at DP_LR; step 0 also against one process at batch 2.
B. vae + kl_free_bits, vae + annealed KL weight (three steps, the first at weight 0), autoencoder + lambda_msssim, cyclevae +
   lambda_swd with per-rank seeds, cyclevaegan with every option it accepts but the image pool.

VCG_BUCKET_MB per case (dp.BUCKET_MB) is the largest power of two that cuts every optimizer into >= 3 buckets: asserted from the
ranks' own plans, and from parallel._Plan at twice the size.

Measured on an MI355X box with 16 CPUs.  Relative L2 distance between 0.5 x the exchanged gradient and the batch-2 gradient at
step 0 (bound GRAD_BOUND = 2e-2; the same on both ranks), and wall time per test (test_gpu_dp_options.py's figures on its box:
13 - 30 s, the cyclevaegan options test 29 s):
    doubleae            optimizer    1.8e-7                              13.8 s
    doublevae           optimizer    4.7e-7                              13.7 s
    cycleae-paired      optimizer    5.3e-7                              18.2 s
    cyclevae            optimizer    5.6e-7                              18.8 s
    aegan               optimizer_G  2.4e-3    optimizer_D  8.0e-4       10.5 s
    vaegan              optimizer_G  3.4e-3    optimizer_D  1.0e-7       10.6 s
    cycleaegan          optimizer_G  3.6e-3    optimizer_D  2.9e-4       18.2 s
    cyclevaegan-paired  optimizer_G  1.16e-2   optimizer_D  2.5e-4       18.7 s
    free bits 9.7 s, anneal 11.0 s, msssim 8.9 s, swd 16.2 s, everything at once 20.6 s; the whole file 192 s.
cyclevaegan-paired's 1.16e-2 is above a third of the bound (the unpaired model measures 7.0e-3, test_gpu_dp_options.py).  By
parameter: the two encoders carry 94.5 % of the squared distance (G.encoder 53.5 %, F.encoder 41.0 %), every encoder layer at
the same relative distance (1.05e-2 in G, 1.36e-2 in F: model.0 .. model.5, weights alike), the decoders 1.8 % and the
bottleneck blocks the rest.  A distance that is uniform over a whole encoder enters above it: the gradient that arrives at the
encoder's output has passed the other generator and this one's decoder, through ReLU masks that the shards (other launch plans
than the batch of two) set differently in a few places, and every encoder layer inherits it; paired, G and F are differentiated
through a third forward (the identity pass), which adds to it.  The bitwise sum above is what holds the wiring; this distance
only says that the shards and the batch of two are two evaluations of one gradient.

The deliberate break (GradReducer._order_after without its wait_stream calls, tried once on a scratch copy) fails
test_two_rank_step_is_the_sum_of_the_shards_alone[aegan] with "aegan step 1 rank 0: optimizer_D.flat_grad is not the sum of the
shards' gradients in 134208 of 2887620 elements (largest difference 8.114e-01)" and test_every_option_at_once_under_two_ranks with
"cyclevaegan step 1 rank 0: optimizer_G.flat_grad is not the sum of the shards' gradients in 9408 of 132432776 elements".

Free bits, step 0: floor 2408.38 (14 of 64 channels have shard 0 above and shard 1 at or below it), loss_kl_fb 2838.476 = the
mean of the shards alone, against 2681.778 for the batch of two (5.8e-2 apart); loss_kl 2225.392, kl_active 0.4375.
"""
import shutil
import time

import pytest
import torch

import test_gpu_dp_options as dp
from conftest import SEED
from test_gpu_dp_options import DP_LR, GRAD_BOUND, LAMBDAS, LR, STEPS, _bits, _check_metrics

pytestmark = pytest.mark.gpu

ARCH_CASES = ["doubleae", "doublevae", "cycleae-paired", "cyclevae", "aegan", "vaegan", "cycleaegan", "cyclevaegan-paired"]
CLIP_KEYS = ("grad_norm", "grad_skipped")          # what the optimizer step leaves: the same on every rank, no mean of shards
ANNEAL = dict(kl_anneal_steps=4, kl_cycles=2, kl_ramp=0.5)


# ------------------------------------------------------------------ the contract, one step
def _plain_model(pkg, case, device, lr, opt_kw, loss_kw, synth=False):
    return dp._configured(pkg, case, device, lr, opt_kw, loss_kw, synth=synth)


def _swd_kw(pkg, loss_kw, rank):
    return dict(loss_kw, swd_seed=pkg.ops.rank_seed(SEED, rank) % 2 ** 32)


def _shard_alone(pkg, model, case, step, rank, before, device, reconfigure=None):
    """training_step on shard `rank` alone, from the state rank `rank` held before the step -> (metrics, {optimizer: flat_grad},
    the model's buffers after the step)"""
    if reconfigure is not None:
        reconfigure(model, rank)                         # the rank's own seeds
    dp._restore(model, before)
    dp._inject_eps(pkg, case, step, slice(rank, rank + 1))
    m = model.training_step(dp._batch(pkg, case, step, device, slice(rank, rank + 1)))
    torch.cuda.synchronize()
    return (m, {n: getattr(model, n).flat_grad.detach().cpu() for n in model._opt_names},
            {k: v.detach().cpu().clone() for k, v in model.named_buffers()})


def _check_step(pkg, model, case, i, step, before, after, buckets, device, reconfigure=None):
    """§1 of the file's docstring for step number `i` (synth stream `step`): `before` / `after` are the two ranks' records.
    Returns the plain runs' metrics."""
    names = dp._opt_names(case)
    dp._assert_replicas(after[0], after[1], names, f"{case} step {i}")
    for r in range(2):
        dp._assert_launches(after[r]["log"], buckets, "start" if i == 0 else "backward", f"{case} step {i} rank {r}")
    alone = [_shard_alone(pkg, model, case, step, r, before[r], device, reconfigure) for r in range(2)]
    (m0, g0, _), (m1, g1, _) = alone
    for r, rec in enumerate(after):
        what = f"{case} step {i} rank {r}"
        # what no optimizer holds (spectral norm's u and v) went the way of the shard alone, and the counters agree
        assert list(rec["extras"]["buffers"]) == list(alone[r][2]), what
        for k, v in alone[r][2].items():
            assert torch.equal(rec["extras"]["buffers"][k], v), f"{what}: buffer {k} differs from the plain run's"
        assert {k: v for k, v in rec["extras"].items() if k not in ("buffers", "swd")} == \
            {k: v for k, v in after[0]["extras"].items() if k not in ("buffers", "swd")}, what
        for n in names:
            want, got = g0[n] + g1[n], rec[f"{n}.flat_grad"]
            assert torch.equal(_bits(got), _bits(want)), \
                f"{what}: {n}.flat_grad is not the sum of the shards' gradients in {(_bits(got) != _bits(want)).sum().item()} of " \
                f"{got.numel()} elements (largest difference {(got - want).abs().max().item():.3e})"
            assert got.abs().max().item() > 0.0, f"{what}: {n}.flat_grad is all zeros"
        m = rec["metrics"]
        assert list(m) == list(m0) == list(m1), f"{what}: metric keys {list(m)} vs the plain runs' {list(m0)}"
        for k, v in m.items():
            if k.startswith(CLIP_KEYS):
                continue
            mean = 0.5 * (m0[k] + m1[k])
            assert abs(v - mean) <= 1e-6 * abs(mean), f"{what}: {k} = {v!r}, the shards alone report {m0[k]!r} and {m1[k]!r}, mean {mean!r}"
    assert after[0]["metrics"] == after[1]["metrics"], f"{case} step {i}: the ranks report different metrics"

    # the summed gradient through a plain optimizer step at 1/2
    dp._restore(model, before[0])
    for n in names:
        opt = getattr(model, n)
        opt.zero_grad()
        opt.flat_grad.copy_(after[0][f"{n}.flat_grad"])
        opt.grad_scale = 0.5
        opt.step()
    torch.cuda.synchronize()
    for n in names:
        opt = getattr(model, n)
        for buf in dp.REPLICATED:
            want, got = getattr(opt, buf, None), after[0][f"{n}.{buf}"]
            assert (want is None) == (got is None), (case, i, n, buf)
            if want is not None:
                want = want.detach().cpu()
                assert torch.equal(_bits(got), _bits(want)), \
                    f"{case} step {i}: the ranks' {n}.{buf} is not what a plain step of the summed gradient at 1/2 leaves: " \
                    f"{(_bits(got) != _bits(want)).sum().item()} of {got.numel()} elements differ"
        if opt.clip_state is not None:
            cs = opt.clip_state.cpu()
            sfx = n[len("optimizer"):]
            assert after[0]["metrics"]["grad_norm" + sfx] == float(cs[0]) and after[0]["metrics"]["grad_skipped" + sfx] == 0.0, \
                (case, i, n, after[0]["metrics"], cs)
        opt.grad_scale = 1.0
    assert not torch.equal(_bits(after[0][f"{names[0]}.flat_param"]), _bits(before[0][f"{names[0]}.flat_param"])), \
        f"{case} step {i}: the step moved no parameter"
    return m0, m1


def _buckets(pkg, cfg, model, case):
    """the ranks' bucket counts: >= 3 per optimizer, and at twice VCG_BUCKET_MB some optimizer would have fewer"""
    metas = [dp._load(cfg, r, "meta") for r in range(2)]
    for meta in metas:
        assert all(v == 0.5 for v in meta["scale"].values()), meta
    buckets = metas[0]["buckets"]
    assert metas[1]["buckets"] == buckets and all(k >= 3 for k in buckets.values()), f"fewer than 3 buckets: {buckets}"
    elems = int(dp.BUCKET_MB[case] * (1 << 20)) // 4
    for n in model._opt_names:
        assert len(pkg.parallel._Plan(getattr(model, n), elems).buckets) == buckets[n], (case, n, buckets)
    twice = {n: len(pkg.parallel._Plan(getattr(model, n), 2 * elems).buckets) for n in model._opt_names}
    assert min(twice.values()) < 3, f"{case}: VCG_BUCKET_MB = {2 * dp.BUCKET_MB[case]} would still give {twice}"
    return buckets


def _run_case(pkg, device, tmp_path, case, tag, lr, steps, opt_kw=None, loss_kw=None, swd=False, model=None, each_step=None):
    """One spawn and §1 on every step.  `each_step(i, after, m0, m1)`: the case's own assertions.  -> (cfg, model, buckets)"""
    opt_kw, loss_kw = opt_kw or {}, loss_kw or {}
    cfg = dp._cfg(case, tmp_path, tag=tag, lr=lr, opt_kw=opt_kw, loss_kw=loss_kw, steps=steps, swd=swd, state=True)
    dp._run_two_ranks(cfg)
    if model is None:
        model = _plain_model(pkg, case, device, lr, opt_kw, _swd_kw(pkg, loss_kw, 0) if swd else loss_kw)
    reconfigure = None
    if swd:
        def reconfigure(m, rank):
            m.configure_loss(**LAMBDAS, **_swd_kw(pkg, loss_kw, rank))
    buckets = _buckets(pkg, cfg, model, case)
    before = [dp._load(cfg, r, "init") for r in range(2)]
    dp._assert_replicas(before[0], before[1], dp._opt_names(case), f"{case} before the first step")
    for i, step in enumerate(steps):
        after = [dp._load(cfg, r, f"step{i}") for r in range(2)]
        m0, m1 = _check_step(pkg, model, case, i, step, before, after, buckets, device, reconfigure)
        if each_step is not None:
            each_step(i, before, after, m0, m1)
        before = after
    return cfg, model, buckets


# ------------------------------------------------------------------ A. the architectures, every option off
@pytest.mark.parametrize("case", ARCH_CASES)
def test_two_rank_step_is_the_sum_of_the_shards_alone(case, pkg, device, tmp_path):
    t0 = time.monotonic()
    names = dp._opt_names(case)
    steps = STEPS[:2]
    kept = {}

    def keep_step0(i, before, after, m0, m1):
        if i == 0:
            wanted = ["metrics"] + [f"{n}.{buf}" for n in names for buf in ("flat_grad", "flat_param")]
            kept.update(before=before[0], after=[{k: rec[k] for k in wanted} for rec in after])

    try:
        cfg, model, _ = _run_case(pkg, device, tmp_path, case, "arch", DP_LR, steps, each_step=keep_step0)
        # step 0 against one process at batch 2 of the same build: same weights, images and eps, no reducer
        dp._restore(model, kept["before"])
        dp._inject_eps(pkg, case, steps[0])
        big = model.training_step(dp._batch(pkg, case, steps[0], device))
        torch.cuda.synchronize()
        for r, rec in enumerate(kept["after"]):
            what = f"{case} step 0 rank {r}"
            _check_metrics(rec["metrics"], big, f"{what}: 2 ranks x batch 1 vs batch 2", tol=1e-4)
            for n in names:
                opt = getattr(model, n)
                err = dp._grad_distance(rec[f"{n}.flat_grad"], opt.flat_grad.cpu())
                print(f"{what} {n}: 0.5 x exchanged gradient vs batch 2: {err:.3e} (bound {GRAD_BOUND:g})")
                assert err <= GRAD_BOUND, f"{what} {n}: averaged shard gradients differ from the big-batch gradient by {err:.2e}"
                moved = (rec[f"{n}.flat_param"] - opt.flat_param.cpu()).abs().max().item()
                assert moved <= 2.5 * DP_LR, f"{what} {n}: parameters differ from the big batch's by {moved:.2e}"
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time architectures[{case}]: {time.monotonic() - t0:.1f} s")


# ------------------------------------------------------------------ B. the newer options
def _channel_kl(pkg, mu, logvar):
    """the KL_c the free-bits gate decides on (fp32, as the device holds them), as float64"""
    return pkg.ops.kl_free_bits(mu, logvar, 0.0, channel_kl=True)[3].double().cpu()


def test_free_bits_floor_acts_on_each_ranks_own_batch(pkg, device, tmp_path):
    """"the floor acts on each rank's own batch".  The floored term is a maximum over a batch mean, so two ranks of
    batch 1 are by design not the batch of two; the floor is chosen, from the shards' own channel KLs, where that shows most."""
    t0 = time.monotonic()
    case, steps = "vae", STEPS[:2]
    model = _plain_model(pkg, case, device, LR, {}, {}, synth=True)
    x = dp._batch(pkg, case, steps[0], device)["x"]
    with torch.no_grad():
        k0, k1 = (_channel_kl(pkg, *model.latent(x[r:r + 1])) for r in range(2))
        mu2, lv2 = model.latent(x)

        def gap(f):
            """(mean of the shards' floored terms, the batch of two's), the batch of two's channel KL being the shards' mean"""
            return 0.5 * (k0.clamp(min=f).mean() + k1.clamp(min=f).mean()).item(), (0.5 * (k0 + k1)).clamp(min=f).mean().item()

        floors = [0.5 * (a + b).item() for a, b in zip(k0, k1) if a > b]
        assert floors, "shard 0 is above shard 1 on no latent channel"
        floor = max(floors, key=lambda f: gap(f)[0] - gap(f)[1])
        split = [(a.item(), b.item()) for a, b in zip(k0, k1) if a > floor >= b]
        dp_fb, big_fb = gap(floor)
        print(f"free bits: floor {floor:.6f}; {len(split)} channel(s) with shard 0 above and shard 1 at or below it, first {split[:1]}; "
              f"floored term: mean of the shards {dp_fb:.6f}, batch of two {big_fb:.6f}")
        # about the inputs, before anything is spawned
        assert split, f"no latent channel has shard 0 above the floor {floor} and shard 1 at or below it"
        assert dp_fb - big_fb > 2e-4 * big_fb, f"the floor {floor} does not tell the shards' mean {dp_fb} from the batch of two {big_fb}"
        big_dev = float(pkg.ops.kl_free_bits(mu2, lv2, floor)[0])          # the batch of two's floored term, by the kernel itself
    loss_kw = dict(kl_free_bits=floor)
    model.configure_loss(**LAMBDAS, **loss_kw)

    def floored(i, before, after, m0, m1):
        for rec in after:
            m = rec["metrics"]
            keys = list(m)
            assert keys[keys.index("loss_kl") + 1:keys.index("loss_kl") + 3] == ["loss_kl_fb", "kl_active"], keys
            for k in ("loss_kl_fb", "kl_active", "loss_kl"):            # (the mean of the shards alone: _check_step; here by name)
                mean = 0.5 * (m0[k] + m1[k])
                assert abs(m[k] - mean) <= 1e-6 * abs(mean), (i, k, m[k], m0[k], m1[k])
            if i == 0:                                                  # the state the floor was chosen at
                print(f"free bits step 0: loss_kl {m['loss_kl']!r} loss_kl_fb {m['loss_kl_fb']!r} kl_active {m['kl_active']!r}; "
                      f"batch of two {big_dev!r}")
                assert abs(m["loss_kl_fb"] - dp_fb) <= 1e-5 * dp_fb, (m["loss_kl_fb"], dp_fb)
                assert abs(m["loss_kl_fb"] - big_dev) > 1e-4 * big_dev, \
                    f"loss_kl_fb {m['loss_kl_fb']!r} is the batch of two's {big_dev!r}: the floor did not act per rank"
                # loss_kl stays the plain mean: float64 over the channel KLs (fp32 values, a fixed fp32 tree over 64 of them)
                plain = 0.5 * (k0.mean() + k1.mean()).item()
                assert abs(m["loss_kl"] - plain) <= 1e-5 * plain, (m["loss_kl"], plain)
                active = int((k0 > floor).sum() + (k1 > floor).sum())
                assert abs(m["kl_active"] * 2 * k0.numel() - active) < 1e-3, (m["kl_active"], active)
    
    try:
        _run_case(pkg, device, tmp_path, case, "freebits", LR, steps, loss_kw=loss_kw, model=model, each_step=floored)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time free_bits: {time.monotonic() - t0:.1f} s")


def test_annealed_kl_weight_is_the_same_on_both_ranks_and_keeps_the_report_counts(pkg, device, tmp_path):
    """Three steps of the cyclical schedule; the first backward, the one the reducer learns its report counts from, runs at
    weight 0.  Every bucket of steps 1 and 2 is still launched from inside the backward (_check_step): a zero-weight step that
    reported fewer gradients would make the reducer raise in step 1."""
    t0 = time.monotonic()
    case, lam = "vae", LAMBDAS["lambda_kl"]
    at = pkg.optim.kl_weight_at
    want = [at(lam, t, ANNEAL["kl_anneal_steps"], ANNEAL["kl_cycles"], ANNEAL["kl_ramp"]) for t in range(3)]
    assert want == [0.0, 0.5 * lam, lam], want                          # host arithmetic: (t / 4) / 0.5, capped at 1

    def weight(i, before, after, m0, m1):
        for rec in after:
            m = rec["metrics"]
            keys = list(m)
            assert keys[keys.index("loss_kl") + 1] == "kl_weight", keys
            assert m["kl_weight"] == want[i] == m0["kl_weight"] == m1["kl_weight"], (i, m["kl_weight"], want[i])
            assert rec["extras"]["steps"]["optimizer"] == [i + 1] * len(rec["extras"]["steps"]["optimizer"])

    try:
        _run_case(pkg, device, tmp_path, case, "anneal", LR, STEPS, loss_kw=dict(ANNEAL), each_step=weight)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time anneal: {time.monotonic() - t0:.1f} s")


def test_multi_scale_ssim_term_under_two_ranks(pkg, device, tmp_path):
    t0 = time.monotonic()
    assert pkg.ops.msssim_max_scales(64, 64) >= 2                       # 64 >> 1 = 32 >= 11

    def reported(i, before, after, m0, m1):
        for rec in after:
            assert list(rec["metrics"])[-1] == "loss_msssim" and rec["metrics"]["loss_msssim"] > 0.0, rec["metrics"]
        assert abs(m0["loss_msssim"] - m1["loss_msssim"]) > 1e-4 * m0["loss_msssim"]      # a rank's own value is not the mean

    try:
        _run_case(pkg, device, tmp_path, "autoencoder", "msssim", LR, STEPS[:2], loss_kw=dict(lambda_msssim=0.5, msssim_scales=2),
                  each_step=reported)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time msssim: {time.monotonic() - t0:.1f} s")


def _assert_swd_plans_differ(pkg, size, levels, calls):
    """host arithmetic: the two ranks' seeds, hence the keys of their direction streams, and their patch offsets differ"""
    L = pkg.Losses.SlicedWassersteinLoss
    fns = [L(levels=levels, seed=pkg.ops.rank_seed(SEED, r) % 2 ** 32) for r in range(2)]
    assert fns[0].seed != fns[1].seed and (L.DIRECTION_STREAM ^ fns[0].seed) != (L.DIRECTION_STREAM ^ fns[1].seed)
    offsets = [[fn.offsets(1, size, size, step=t) for t in range(calls)] for fn in fns]
    assert offsets[0] != offsets[1], f"the two ranks draw the same patch offsets: {offsets[0]}"
    return fns


def _swd_each_step(pkg, device, fns, calls_per_step):
    def check(i, before, after, m0, m1):
        for r, rec in enumerate(after):
            assert "loss_swd" in rec["metrics"] and rec["metrics"]["loss_swd"] > 0.0, rec["metrics"]
            # the counter advanced equally, each rank under its own seed
            assert rec["extras"]["swd"]["_extra_state"] == {"seed": fns[r].seed, "step": calls_per_step * (i + 1), "levels": fns[r].levels}
        if i == 0:
            d0, d1 = (fn.directions(device, step=0).cpu() for fn in fns)
            assert not torch.equal(d0, d1), "the two ranks drew the same directions"
            assert abs(m0["loss_swd"] - m1["loss_swd"]) > 1e-4 * m0["loss_swd"]
    return check


def test_sliced_wasserstein_term_draws_a_plan_per_rank(pkg, device, tmp_path):
    """cyclevae, unpaired: loss_swd is the mean of the shards alone under THEIR seeds, the counter advances by the step's two
    evaluations on both ranks, and the exchanged gradient is the sum of the shards' on both steps."""
    t0 = time.monotonic()
    steps = STEPS[:2]
    fns = _assert_swd_plans_differ(pkg, 64, 3, 2 * len(steps))
    try:
        _run_case(pkg, device, tmp_path, "cyclevae", "swd", LR, steps, loss_kw=dict(lambda_swd=1.0, swd_levels=3), swd=True,
                  each_step=_swd_each_step(pkg, device, fns, 2))
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time swd: {time.monotonic() - t0:.1f} s")


def test_every_option_at_once_under_two_ranks(pkg, device, tmp_path):
    """cyclevaegan, unpaired, with everything it accepts but the image pool (test_image_pool_under_two_ranks): the four image
    terms at the scales 256 x 256 allows, the sliced Wasserstein term with per-rank seeds, the free-bits floor (the median of
    shard 0's own channel KLs), the annealed weight (step 0 at weight 0), clipping and the average."""
    t0 = time.monotonic()
    case, steps = "cyclevaegan", STEPS[:2]
    assert pkg.ops.msssim_max_scales(256, 256) == 5
    fns = _assert_swd_plans_differ(pkg, 256, 3, 2 * len(steps))
    opt_kw = dict(clip_grad_norm=dp.CLIP[case], ema_decay=dp.EMA_DECAY)
    model = _plain_model(pkg, case, device, LR, opt_kw, {}, synth=True)
    seen = []
    handle = model.loss_kl.register_forward_hook(lambda mod, inp, out: seen.append(inp))
    model.eval()
    dp._inject_eps(pkg, case, steps[0], slice(0, 1))
    with torch.no_grad():
        model.validation_step(dp._batch(pkg, case, steps[0], device, slice(0, 1)))
        kls = torch.cat([_channel_kl(pkg, mu, lv) for mu, lv in seen]).sort().values
    handle.remove()
    model.train()
    assert len(kls) == 4 * 64
    floor = 0.5 * (kls[len(kls) // 2 - 1] + kls[len(kls) // 2]).item()
    assert kls[0] < floor < kls[-1], (kls[0], floor, kls[-1])
    loss_kw = dict(lambda_ssim=0.5, lambda_grad=0.5, lambda_freq=0.5, lambda_msssim=0.5, grad_scales=4, msssim_scales=5,
                   lambda_swd=1.0, swd_levels=3, kl_free_bits=floor, **ANNEAL)
    swd_check = _swd_each_step(pkg, device, fns, 2)
    lam = LAMBDAS["lambda_kl"]

    def everything(i, before, after, m0, m1):
        swd_check(i, before, after, m0, m1)
        for rec in after:
            m = rec["metrics"]
            assert all(k in m for k in ("loss_ssim", "loss_grad", "loss_freq", "loss_msssim", "loss_swd", "loss_kl_fb", "kl_active",
                                        "kl_weight", "grad_norm_G", "grad_norm_D")), list(m)
            assert m["kl_weight"] == [0.0, 0.5 * lam][i] and 0.0 < m["kl_active"] < 1.0, (i, m["kl_weight"], m["kl_active"])
            assert rec["optimizer_G.flat_ema"] is not None and rec["optimizer_D.flat_ema"] is None
            assert rec["extras"]["ema_updates"]["optimizer_G"] == i + 1

    try:
        _run_case(pkg, device, tmp_path, case, "all", LR, steps, opt_kw=opt_kw, loss_kw=loss_kw, swd=True, model=model,
                  each_step=everything)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time all_on: {time.monotonic() - t0:.1f} s")
