"""GPU: the data-parallel step (parallel.GradReducer) together with the step options that were merged after it was last tested:
clip_grad_norm, ema_decay, lambda_ssim and pool_size.  train.py hands all of them to a model that also carries a reducer; every
other test of the options is single-process, and the two-rank test of tests/test_gpu_parity.py runs with all of them off.

The set-up is _dp_gpu_worker's of test_gpu_parity.py: two ranks share the one card with a batch of 1 each, gloo carries the
exchange, the weights are pkg.synth.state_dict_like's, batches and eps are the rows of pkg.synth.batch(2, ...) / eps_list.  BOTH
ranks write what they hold after every step (metrics, flat_grad / flat_param / exp_avg / exp_avg_sq / flat_ema / clip_state of
every optimizer, the reducer's log), one file per rank and step, and the parent checks the files.

1. test_options_on_equal_the_big_batch_and_their_definitions (autoencoder, vae, cyclevaegan): three steps at the training lr with
   clipping, EMA and SSIM on, rank 1 starting from OTHER weights and a forward of its own before parallel.broadcast_parameters.
   Replicas stay bitwise equal; step 0 equals one process at batch 2; clip_state follows its float64 definition over the rank's
   own exchanged gradient; the first moment shows the clip coefficient; the average copies, then follows the fma recurrence;
   steps 1 and 2 exchange every bucket from inside the backward.
2. test_image_pool_under_two_ranks (cyclevaegan): pool_size=1 with train.py's per-rank pool seeds.  The plans are asserted first;
   step 1 is an identity plan that drew (the extra discriminator call exists only under a reducer), in step 2 the ranks differ.
   Against the same ranks with every bucket exchanged after the backward (bitwise), and step 1 against one process at batch 2
   whose pools are a stub that shows the two ranks' recorded images.
3. test_a_nan_on_one_rank_skips_the_step_on_both (vae: device-side skip; autoencoder: host guard through any_rank): the NaN
   reaches rank 0 only through the sum.

Trouble ends a test: the process group gets a 60 s timeout, the ranks are `spawn` processes joined under a limit, and a rank that
dies or a limit that expires terminates both.  At most the parent and two ranks have the card open.

Wall time per test on an MI355X box with 16 CPUs: options 16 s (autoencoder), 15 s (vae), 29 s (cyclevaegan); image pool 30 s (two
spawns); NaN 13 s each.  A two-rank spawn is 7 s (64 x 64 models) to 11 s (cyclevaegan), of which 2 - 4 s pass before the model
exists (process start, import, synthesised weights), each step is 0.1 - 0.5 s and writing its record 0.6 - 1.2 s; the rest of a
test is the parent's float64 arithmetic over the records and its own batch-2 model."""
import multiprocessing.connection
import os
import shutil
import socket
import sys
import time
from datetime import timedelta

import numpy as np
import pytest
import torch

from conftest import SEED
from test_gpu_parity import DP_LR, LAMBDAS, LR, STEP_BIAS_STD, _check_metrics, load_synth, nchw

pytestmark = pytest.mark.gpu

# The tables below are keyed by case: an architecture of train.py, "-paired" appended for a cycle model with paired=True (a bare
# cycle name is the unpaired model).  tests/test_gpu_dp_architectures.py runs the cases this file's own tests do not.
GAN_ARCHS = ("aegan", "vaegan", "cycleaegan", "cyclevaegan")       # train.POOL_ARCHS: optimizer_G and optimizer_D
SMALL = ("autoencoder", "vae", "doubleae", "doublevae", "cycleae-paired", "cyclevae")
LARGE = ("aegan", "vaegan", "cycleaegan", "cyclevaegan", "cyclevaegan-paired")
# the smallest the goldens use; the discriminators' 16 x 16 full-map layer admits nothing below 256
SIZE = {**{c: 64 for c in SMALL}, **{c: 256 for c in LARGE}}
# the weight streams of the golden steps
SYNTH_KEY = {"autoencoder": "ae64", "vae": "vae64", "cyclevaegan": "dp", "doubleae": "dae64", "doublevae": "dve64",
             "cycleae-paired": "cae64_paired", "cyclevae": "cve64_unpaired", "aegan": "aeg256", "vaegan": "vag256",
             "cycleaegan": "cag256_unpaired", "cyclevaegan-paired": "cvg256_paired"}
STEPS = (3, 4, 5)                      # synth batch / eps stream indices (3, 4: the existing two-rank test's)
# VCG_BUCKET_MB per model: the largest power of two that still cuts every optimizer into >= 3 buckets (asserted).  Autoencoder
# 245.7 MiB -> 4 buckets, VAE 252.6 MiB -> 4, CycleVAEGAN optimizer_G 505.2 MiB -> 14 and optimizer_D 22.0 MiB -> 3
# DoubleAE 323.7 MiB -> 3, DoubleVAE 337.5 -> 3, CycleAE 491.4 -> 4, CycleVAE 505.2 -> 4; AEGAN optimizer_G 245.7 -> 9 and
# optimizer_D 11.0 -> 3, VAEGAN 252.6 -> 12 and 11.0 -> 3, CycleAEGAN 491.4 -> 14 and 22.0 -> 3
BUCKET_MB = {"autoencoder": 64, "vae": 64, "cyclevaegan": 8, "doubleae": 128, "doublevae": 128, "cycleae-paired": 128,
             "cyclevae": 128, "aegan": 2, "vaegan": 2, "cycleaegan": 8, "cyclevaegan-paired": 8}
EMA_DECAY = 0.999
LAMBDA_SSIM = 0.5
BETA1 = 0.5                            # configure_optimizers' default betas (0.5, 0.999)
# clip_grad_norm per model: one power of two below half of the smallest norm the batch-2 run of the commit before this file
# reports at these inputs (options on, bound 1e30 so that it measures and clips nothing), steps 0 / 1 / 2:
#   autoencoder  grad_norm      31.65 /   29.52 /   30.27   -> 8
#   vae          grad_norm      54.04 /   49.12 /   52.84   -> 16
#   cyclevaegan  grad_norm_G  3732.30 / 3187.67 / 2507.42
#                grad_norm_D   284.13 /  159.90 /  267.89   -> 64 (one bound, two norms: below half of the discriminators')
CLIP = {"autoencoder": 8.0, "vae": 16.0, "cyclevaegan": 64.0}
GRAD_BOUND = 2e-2                      # test_two_rank_step_equals_the_big_batch_step's: a wiring error is O(1) on a bucket
# measured relative L2 distance between 0.5 x the exchanged gradient and the batch-2 gradient (bound 2e-2):
#   autoencoder 1.2e-7, vae 2.1e-7, cyclevaegan optimizer_G 7.0e-3 and optimizer_D 2.7e-4, the same on both ranks.  The
#   generators' 7.0e-3 is above a third of the bound; it is the distance test_two_rank_step_equals_the_big_batch_step measures
#   with every option off (7.2e-3 there: the shards take other launch plans than the batch of two), not something the options add.
#   Image pool test, step 1 against the batch of two: optimizer_G 1.34e-2 (the existing test's second step: 1.35e-2), optimizer_D
#   4.2e-7
JOIN_LIMIT = {**{c: 240.0 for c in SMALL}, **{c: 480.0 for c in LARGE}}       # seconds; a healthy run needs a fraction of it
BUFFERS = ("flat_grad", "flat_param", "exp_avg", "exp_avg_sq", "flat_ema", "clip_state")
REPLICATED = ("flat_param", "exp_avg", "exp_avg_sq", "flat_ema", "clip_state")
POOLS = (("DX", "fake_x", "d_fake_x"), ("DY", "fake_y", "d_fake_y"))
# ImagePool.plan with pool_seed = ops.rank_seed(SEED, rank), capacity 1, one image per step: host arithmetic, asserted before
# anything else so that a seed change cannot hollow the pool test out.  [-2] stores (filling), [-1] keeps, [0] swaps with slot 0
PLANS = {0: {"DX": ([-2], [-1], [0]), "DY": ([-2], [0], [0])},
         1: {"DX": ([-2], [-1], [-1]), "DY": ([-2], [0], [0])}}


# ------------------------------------------------------------------ shared by the ranks and the one-process runs
def _base(case):
    return case.split("-")[0]


def _make_model(pkg, case):
    N, paired = pkg.Networks, case.endswith("-paired")
    return {"autoencoder": lambda: N.Autoencoder(), "vae": lambda: N.VariationalAutoencoder(latent_dim=64),
            "doubleae": lambda: N.DoubleAutoencoder(), "doublevae": lambda: N.DoubleVariationalAutoencoder(latent_dim=64),
            "cycleae": lambda: N.CycleAE(paired=paired), "cyclevae": lambda: N.CycleVAE(latent_dim=64, paired=paired),
            "aegan": lambda: N.AEGAN(), "vaegan": lambda: N.VAEGAN(latent_dim=64),
            "cycleaegan": lambda: N.CycleAEGAN(paired=paired),
            "cyclevaegan": lambda: N.CycleVAEGAN(latent_dim=64, paired=paired)}[_base(case)]()


def _batch(pkg, arch, step, dev, rows=slice(None)):
    x, y = pkg.synth.batch(2, SIZE[arch], SEED, step=step)
    xb = torch.from_numpy(x[rows]).to(dev)
    return {"x": xb, "y": xb if arch in ("autoencoder", "vae") else torch.from_numpy(y[rows]).to(dev)}


# eps draws of one training step at batch 2, in the reference's call order: doublevae block A, block B; cyclevae G(x), F(G(x)),
# F(y), G(F(y)); vaegan G(x), G(y); cyclevaegan G(x), G(y), F(G(x)), F(y), F(x), G(F(y)) (unpaired: the identity draws are skipped)
EPS_DRAWS = {"vae": (1, (2, 64, 4, 4)), "doublevae": (2, (2, 64, 4, 4)), "cyclevae": (4, (2, 64, 4, 4)),
             "vaegan": (2, (2, 64, 16, 16)), "cyclevaegan": (6, (2, 64, 16, 16))}


def _inject_eps(pkg, arch, step, rows=slice(None)):
    if _base(arch) not in EPS_DRAWS:
        return
    count, shape = EPS_DRAWS[_base(arch)]
    pkg.ops.inject_eps([torch.from_numpy(e[rows]) for e in pkg.synth.eps_list(count, shape, SEED, step=step)])


def _configured(pkg, arch, dev, lr, opt_kw, loss_kw, seed=SEED, synth=True):
    model = _make_model(pkg, arch)
    if synth:                                    # False: the caller loads a recorded state (_restore) before the first step
        load_synth(pkg, model, SYNTH_KEY[arch], STEP_BIAS_STD, seed=seed)
    model = model.to(dev).train()
    model.configure_optimizers(lr=lr, **opt_kw)
    model.configure_loss(**LAMBDAS, **loss_kw)
    return model


def _record(model, metrics, buffers):
    torch.cuda.synchronize()
    rec = {"metrics": metrics}
    for name in model._opt_names:
        opt = getattr(model, name)
        for buf in buffers:
            t = getattr(opt, buf, None)
            rec[f"{name}.{buf}"] = None if t is None else t.detach().cpu()
    return rec


def _extras(model):
    """What a step starts from beside the optimizers' flat buffers (_record holds the parameters, both moments and the average as
    flat_param, exp_avg, exp_avg_sq and flat_ema: model.state_dict()'s parameters and save_optimizer_states()'s moments are
    views and clones of exactly these, so they are written once): the buffers no optimizer holds (spectral norm's u and v), the
    step counters, the average's update count, and the sliced Wasserstein term's seed and call counter."""
    opts = {n: getattr(model, n) for n in model._opt_names}
    return {"buffers": {k: v.detach().cpu().clone() for k, v in model.named_buffers()},
            "steps": {n: list(o.steps) for n, o in opts.items()},
            "ema_updates": {n: getattr(o, "ema_updates", None) for n, o in opts.items()},
            "swd": model.save_swd_state() if getattr(model, "swd_term", None) is not None else None}


def _restore(model, rec):
    """Put a plain model of the same case into the state a rank recorded (_record with every buffer of BUFFERS, _extras), through
    the public loaders: load_state_dict, the optimizers' load_state_dict / load_ema_state, load_swd_state."""
    torch.cuda.synchronize()
    names = {id(p): n for n, p in model.named_parameters()}
    opts = {n: getattr(model, n) for n in model._opt_names}

    def views(n, buf):
        flat = rec[f"{n}.{buf}"]
        assert flat.numel() == opts[n].total, (n, buf, flat.numel(), opts[n].total)
        return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(opts[n].params, opts[n].offsets)]

    sd = dict(rec["extras"]["buffers"])
    for n, opt in opts.items():
        sd.update({names[id(p)]: v for p, v in zip(opt.params, views(n, "flat_param"))})
    model.load_state_dict(sd)
    for n, opt in opts.items():
        state = {i: {"step": torch.tensor(float(t)), "exp_avg": a, "exp_avg_sq": b}
                 for i, (t, a, b) in enumerate(zip(rec["extras"]["steps"][n], views(n, "exp_avg"), views(n, "exp_avg_sq"))) if t > 0}
        group = {k: v for k, v in opt.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(opt.params)))
        opt.load_state_dict({"state": state, "param_groups": [group]})
        if opt.flat_ema is not None:
            opt.load_ema_state({"updates": rec["extras"]["ema_updates"][n], "tensors": views(n, "flat_ema")})
        opt.grad_scale = 1.0
    if rec["extras"]["swd"] is not None:
        model.load_swd_state(rec["extras"]["swd"])


# ------------------------------------------------------------------ one rank
def _rank(rank, world, port, cfg):
    """cfg: arch, outdir, tag, lr, opt_kw, loss_kw, from_backward, buffers, ranks_saving, and the scenario switches `diverge`
    (rank 1 loads other weights and runs a forward before the broadcast), `pool`, `nan_steps` (indices of the steps whose input
    on rank 1 holds one NaN pixel), `steps` (the synth batch / eps stream index of every step), `swd` (the sliced Wasserstein
    term's seed is derived per rank, as train.py does), `state` (every record carries _extras, and one more record, "init",
    holds what the rank held before its first step)."""
    import importlib
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    arch = cfg["arch"]
    # two processes share the one card: 4 hardware queues each, not the package's 8 (test_gpu_parity._dp_gpu_worker); this
    # process has not initialised HIP yet, so the setting takes
    os.environ["GPU_MAX_HW_QUEUES"] = "4"
    os.environ["VCG_BUCKET_MB"] = str(BUCKET_MB[arch])
    os.environ["VCG_DP_FROM_BACKWARD"] = "1" if cfg["from_backward"] else "0"
    clock = [("start", time.monotonic())]
    pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}",
                            timeout=timedelta(seconds=60))
    try:
        dev = torch.device("cuda:0")
        opt_kw = dict(cfg["opt_kw"])
        if cfg["pool"]:
            opt_kw.update(pool_size=1, pool_seed=pkg.ops.rank_seed(SEED, rank))      # as train.py derives it
        loss_kw = dict(cfg["loss_kw"])
        if cfg.get("swd"):
            loss_kw.update(swd_seed=pkg.ops.rank_seed(SEED, rank) % 2 ** 32)          # as train.py derives it
        model = _configured(pkg, arch, dev, cfg["lr"], opt_kw, loss_kw,
                            seed=SEED + 1 if cfg["diverge"] and rank == 1 else SEED)
        clock.append(("model", time.monotonic()))
        calls = {}
        if cfg["pool"]:
            model.enable_debug_mode(True)
            for name, _, _ in POOLS:
                getattr(model, name).register_forward_hook(lambda *_, name=name: calls.__setitem__(name, calls.get(name, 0) + 1))
        red = pkg.parallel.attach(model)                     # train.py's order: optimizers, losses, attach, broadcast
        if cfg["diverge"]:
            if rank == 1:                                    # its weight packs exist, built from the weights it is about to lose
                model.eval()
                _inject_eps(pkg, arch, STEPS[0], slice(1, 2))
                model.validation_step(_batch(pkg, arch, STEPS[0], dev, slice(1, 2)))
                model.train()
            pkg.parallel.broadcast_parameters(model)
        clock.append(("broadcast", time.monotonic()))
        save = rank in cfg["ranks_saving"]
        if cfg.get("state") and save:
            rec = _record(model, {}, cfg["buffers"])
            rec["extras"] = _extras(model)
            torch.save(rec, os.path.join(cfg["outdir"], f"{cfg['tag']}_rank{rank}_init.pt"))
            del rec
        for i, step in enumerate(cfg["steps"]):
            batch = _batch(pkg, arch, step, dev, slice(rank, rank + 1))
            if i in cfg["nan_steps"] and rank == 1:
                bad = batch["x"].clone()
                bad[0, 1, 5, 7] = float("nan")
                batch = {"x": bad, "y": bad if arch != "cyclevaegan" else batch["y"]}
            _inject_eps(pkg, arch, step, slice(rank, rank + 1))
            n0 = len(red.log)
            calls.clear()
            m = model.training_step(batch)
            torch.cuda.synchronize()
            clock.append((f"step{i}", time.monotonic()))
            rec = _record(model, m, cfg["buffers"])
            rec["log"] = list(red.log[n0:])
            if cfg.get("state"):
                rec["extras"] = _extras(model)
            if cfg["pool"]:
                rec["plans"] = {n: list(p.last_plan) for n, p in model.image_pools.items()}
                rec["drew"] = {n: (p.last_identity, p.last_drew) for n, p in model.image_pools.items()}
                rec["d_calls"] = dict(calls)
                for _, fake, shown in POOLS:
                    rec[fake], rec[shown] = nchw(model.debug_info[fake]), nchw(model.debug_info[shown])
            if save:
                torch.save(rec, os.path.join(cfg["outdir"], f"{cfg['tag']}_rank{rank}_step{i}.pt"))
            del rec
            clock.append((f"saved{i}", time.monotonic()))
        if save:
            meta = {"seconds": [(k, round(t - clock[0][1], 1)) for k, t in clock[1:]],
                    "scale": {n: getattr(model, n).grad_scale for n in model._opt_names},
                    "buckets": {n: len(red._plans[id(getattr(model, n))].buckets) for n in model._opt_names},
                    "ema_updates": {n: getattr(getattr(model, n), "ema_updates", None) for n in model._opt_names}}
            torch.save(meta, os.path.join(cfg["outdir"], f"{cfg['tag']}_rank{rank}_meta.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _cfg(arch, outdir, tag="dp", lr=LR, opt_kw=None, loss_kw=None, from_backward=True, buffers=BUFFERS, ranks_saving=(0, 1),
         diverge=False, pool=False, nan_steps=(), steps=STEPS, swd=False, state=False):
    return dict(arch=arch, outdir=str(outdir), tag=tag, lr=lr, opt_kw=opt_kw or {}, loss_kw=loss_kw or {},
                from_backward=from_backward, buffers=buffers, ranks_saving=ranks_saving, diverge=diverge, pool=pool,
                nan_steps=tuple(nan_steps), steps=tuple(steps), swd=swd, state=state)


def _run_two_ranks(cfg):
    """Two `spawn` processes, joined under JOIN_LIMIT.  A rank that exits with an error, or the limit, terminates both and fails
    the test; nothing is tried again.  Waiting is on the processes' sentinels."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank, args=(rank, 2, port, cfg)) for rank in range(2)]
    limit = JOIN_LIMIT[cfg["arch"]]
    deadline = time.monotonic() + limit
    for p in procs:
        p.start()
    trouble = None
    try:
        while trouble is None:
            codes = [p.exitcode for p in procs]
            if all(c == 0 for c in codes):
                break
            if any(c not in (None, 0) for c in codes):
                trouble = f"exit codes {codes} (None: still running when the other rank failed)"
                break
            left = deadline - time.monotonic()
            if left <= 0:
                trouble = f"not finished after {limit:.0f} s (exit codes {codes}): a rank hangs"
                break
            # woken by a rank's exit; the cap only bounds the wait should a sentinel stay silent after its process has gone
            multiprocessing.connection.wait([p.sentinel for p in procs if p.exitcode is None], timeout=min(left, 1.0))
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(10)
            if p.is_alive():
                p.kill()
                p.join(10)
    if trouble is not None:
        pytest.fail(f"two-rank {cfg['arch']} run '{cfg['tag']}': {trouble}")
    seconds = _load(cfg, min(cfg["ranks_saving"]), "meta")["seconds"]
    print(f"two-rank {cfg['arch']} run '{cfg['tag']}': {time.monotonic() - (deadline - limit):.1f} s; inside rank {min(cfg['ranks_saving'])}: {seconds}")


def _load(cfg, rank, what):
    return torch.load(os.path.join(cfg["outdir"], f"{cfg['tag']}_rank{rank}_{what}.pt"), weights_only=False)


def _bits(t):
    return t.view(torch.int32)


def _sfx(name):
    return name[len("optimizer"):]


def _assert_replicas(r0, r1, opt_names, what):
    for name in opt_names:
        for buf in REPLICATED:
            a, b = r0.get(f"{name}.{buf}"), r1.get(f"{name}.{buf}")       # None: not kept (no average, no clipping) or not recorded
            assert (a is None) == (b is None), (what, name, buf)
            if a is not None:
                assert torch.equal(_bits(a), _bits(b)), \
                    f"{what}: {name}.{buf} differs between the ranks in {(_bits(a) != _bits(b)).sum().item()} of {a.numel()} elements"


def _assert_launches(log, buckets, where, what):
    """every bucket of every optimizer was exchanged exactly once, all of them from `where`"""
    assert log and all(w == where for *_, w in log), f"{what}: {log}"
    assert sorted((tag, b) for tag, b, *_ in log) == sorted((n, b) for n, k in buckets.items() for b in range(k)), f"{what}: {log}"


def _grad_distance(exchanged, big):
    """relative L2 distance in float64 between 0.5 x the exchanged (summed) gradient and the batch-2 gradient"""
    big = big.double()
    return ((exchanged.double() * 0.5 - big).norm() / big.norm()).item()


def _opt_names(arch):
    return ("optimizer_G", "optimizer_D") if _base(arch) in GAN_ARCHS else ("optimizer",)


# ------------------------------------------------------------------ 1. clipping, EMA and SSIM on
def _check_clip_state(rec, name, c, what):
    """clip_state against its definition in float64 over the rank's own exchanged gradient (grad_scale = 1/2), with the
    per-quantity bounds test_gpu_grad_clip.py holds vcg_grad_norm to; the reported metrics carry its bits."""
    from test_gpu_grad_clip import BOUND, ref_coef
    g = rec[f"{name}.flat_grad"].double()
    norm = 0.5 * float(torch.dot(g, g).sqrt())
    cs = rec[f"{name}.clip_state"].numpy()
    coef = ref_coef(norm, c)
    e0 = abs(float(cs[0]) - norm) / norm
    print(f"{what} {name}: norm {float(cs[0])!r} ({e0:.2e} from float64), coefficient {float(cs[1])!r}")
    assert e0 <= BOUND, f"{what} {name}: clip_state[0] = {cs[0]!r}, 0.5 ||flat_grad|| = {norm!r}: off by {e0:.3e} (bound {BOUND:.3e})"
    assert coef < 1.0, f"{what} {name}: the norm {norm!r} is not above clip_grad_norm = {c}: clipping is inactive and the test checks nothing"
    e1 = abs(float(cs[1]) - coef) / coef
    assert e1 <= BOUND and cs[1] < 1.0, f"{what} {name}: coefficient {cs[1]!r} vs {coef!r}: off by {e1:.3e} (bound {BOUND:.3e})"
    assert cs[2] == 0.0 and cs[3] == 0.0, (what, name, cs)
    m = rec["metrics"]
    assert np.float32(m["grad_norm" + _sfx(name)]).view(np.int32) == cs[:1].view(np.int32)[0], \
        f"{what} {name}: reported grad_norm {m['grad_norm' + _sfx(name)]!r}, clip_state[0] {cs[0]!r}"
    assert m["grad_norm" + _sfx(name)] == float(cs[0]) and m["grad_skipped" + _sfx(name)] == 0.0, (what, name, m)
    return cs


def _check_first_moment(rec, name, cs, what):
    """after the first step exp_avg = (1 - beta1) g fl32(0.5 coefficient): Adam's update is scale-free, so the parameters cannot
    show a wrong coefficient; the first moment can.  Element bound: test_gpu_grad_clip.py's for the clipped Adam step against
    torch (rel L2 1e-6, largest error 2e-6 of the largest element)."""
    s = float(np.float32(np.float32(0.5) * cs[1]))
    want = rec[f"{name}.flat_grad"].double() * ((1.0 - BETA1) * s)
    err = rec[f"{name}.exp_avg"].double() - want
    l2, mx = (err.norm() / want.norm()).item(), (err.abs().max() / want.abs().max()).item()
    print(f"{what} {name}: exp_avg vs (1 - beta1) g fl32(0.5 coef): rel L2 {l2:.2e}, max {mx:.2e}")
    assert l2 <= 1e-6 and mx <= 2e-6, f"{what} {name}: exp_avg is not (1 - beta1) x g x {s!r}: rel L2 {l2:.3e}, max {mx:.3e}"


@pytest.mark.parametrize("arch", ["autoencoder", "vae", "cyclevaegan"])
def test_options_on_equal_the_big_batch_and_their_definitions(arch, pkg, device, tmp_path):
    from test_gpu_ema import check_within_bound
    t0 = time.monotonic()
    c = CLIP[arch]
    opt_kw, loss_kw = dict(clip_grad_norm=c, ema_decay=EMA_DECAY), dict(lambda_ssim=LAMBDA_SSIM)
    cfg = _cfg(arch, tmp_path, opt_kw=opt_kw, loss_kw=loss_kw, diverge=True)
    names = _opt_names(arch)
    try:
        _run_two_ranks(cfg)
        metas = [_load(cfg, r, "meta") for r in range(2)]
        for meta in metas:
            assert all(v == 0.5 for v in meta["scale"].values()), meta
            assert all(k >= 3 for k in meta["buckets"].values()), f"fewer than 3 buckets: {meta['buckets']}"
        buckets = metas[0]["buckets"]

        # one process of this build at batch 2: same weights, images, eps and options, no reducer.  Step 0 does not depend on lr
        model = _configured(pkg, arch, device, LR, opt_kw, loss_kw)
        _inject_eps(pkg, arch, STEPS[0])
        big = _record(model, model.training_step(_batch(pkg, arch, STEPS[0], device)), ("flat_grad",))
        del model

        ema_name = names[0]                              # `optimizer` / `optimizer_G`: the discriminators keep no average
        prev = None
        for i in range(len(STEPS)):
            recs = [_load(cfg, r, f"step{i}") for r in range(2)]
            _assert_replicas(recs[0], recs[1], names, f"{arch} step {i}")
            for r, rec in enumerate(recs):
                what = f"{arch} step {i} rank {r}"
                if i == 0:
                    # metrics to the first-step tolerance of the existing two-rank test, loss_ssim and grad_norm* included
                    assert "loss_ssim" in rec["metrics"] and all("grad_norm" + _sfx(n) in rec["metrics"] for n in names)
                    _check_metrics(rec["metrics"], big["metrics"], f"{what}: 2 ranks x batch 1 vs batch 2", tol=1e-4)
                    _assert_launches(rec["log"], buckets, "start", what)         # the first backward learns the report counts
                else:
                    _assert_launches(rec["log"], buckets, "backward", what)
                for name in names:
                    if i == 0:
                        err = _grad_distance(rec[f"{name}.flat_grad"], big[f"{name}.flat_grad"])
                        print(f"{what} {name}: 0.5 x exchanged gradient vs batch 2: {err:.3e} (bound {GRAD_BOUND:g})")
                        assert err <= GRAD_BOUND, f"{what} {name}: averaged shard gradients differ from the big-batch gradient by {err:.2e}"
                    cs = _check_clip_state(rec, name, c, what)
                    if i == 0:
                        _check_first_moment(rec, name, cs, what)
                assert rec[f"{ema_name}.flat_ema"] is not None and all(rec[f"{n}.flat_ema"] is None for n in names[1:])
            # the average, over rank 0's records: rank 1's parameters and average are these bit for bit (_assert_replicas)
            cur, ema = recs[0][f"{ema_name}.flat_param"], recs[0][f"{ema_name}.flat_ema"]
            if i == 0:
                # the first update copies: what was BROADCAST after the optimizer was built is what the average starts from
                assert torch.equal(_bits(ema), _bits(cur)), f"{arch}: after the first step the average is not the parameters"
            else:
                d = pkg.optim.ema_decay_at(EMA_DECAY, i)
                check_within_bound(ema.numpy(), cur.numpy(), prev.numpy(), 1.0 - d, f"{arch} average after step {i} (decay {d:.4f})")
                assert not torch.equal(_bits(ema), _bits(cur)) and not torch.equal(_bits(ema), _bits(prev))
            prev = ema
            del recs
        assert metas[0]["ema_updates"][ema_name] == metas[1]["ema_updates"][ema_name] == len(STEPS)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time options[{arch}]: {time.monotonic() - t0:.1f} s")


# ------------------------------------------------------------------ 2. image history pools under two ranks
class _RecordedPool:
    """Stands in for image_pool.ImagePool in the one-process run at batch 2: step 0 fills (the batch is shown as it is, no extra
    call), step 1 shows the images the two ranks' pools showed, as a plan that swapped."""

    def __init__(self, shown):
        self.shown = list(shown)                 # per step: None (identity) or the batch to show
        self.last_plan, self.last_identity, self.last_drew = [], True, False

    def exchange(self, fake):
        shown = self.shown.pop(0)
        self.last_identity, self.last_drew = shown is None, shown is not None
        return fake if shown is None else shown


def test_image_pool_under_two_ranks(pkg, device, tmp_path):
    t0 = time.monotonic()
    arch, names = "cyclevaegan", _opt_names("cyclevaegan")
    moments = ("flat_grad", "flat_param", "exp_avg", "exp_avg_sq")
    cfg = _cfg(arch, tmp_path, tag="pool", lr=DP_LR, pool=True, buffers=moments)
    # the same ranks with every bucket exchanged after the backward: rank 0's gradients, parameters and metrics
    ref_cfg = _cfg(arch, tmp_path, tag="pool_at_start", lr=DP_LR, pool=True, from_backward=False,
                   buffers=("flat_grad", "flat_param"), ranks_saving=(0,))
    try:
        _run_two_ranks(cfg)
        metas = [_load(cfg, r, "meta") for r in range(2)]
        buckets = metas[0]["buckets"]
        assert all(k >= 3 for k in buckets.values()) and metas[1]["buckets"] == buckets, buckets
        slot = [{}, {}]                                  # per rank, per pool: what the one slot holds (host mirror)
        shown_step1 = {}
        for i in range(len(STEPS)):
            recs = [_load(cfg, r, f"step{i}") for r in range(2)]
            for r, rec in enumerate(recs):
                what = f"pool step {i} rank {r}"
                # the plans first
                assert rec["plans"] == {n: PLANS[r][n][i] for n in ("DX", "DY")}, f"{what}: plans {rec['plans']}"
                for n, fake, shown in POOLS:
                    plan = rec["plans"][n]
                    identity, drew = rec["drew"][n]
                    assert drew == (i > 0) and identity == (plan != [0]), (what, n, plan, identity, drew)
                    # every rank takes the extra call D(pooled) whenever its pool drew, kept samples included: fake, real, pooled
                    assert rec["d_calls"][n] == (3 if i > 0 else 2), f"{what}: {n} was called {rec['d_calls'][n]} times"
                    if plan == [0]:                      # swapped: the slot's image is shown, this step's fake takes its place
                        assert torch.equal(_bits(rec[shown]), _bits(slot[r][n])), f"{what}: {n} was not shown the stored image"
                        assert not torch.equal(_bits(rec[shown]), _bits(rec[fake]))
                        slot[r][n] = rec[fake]
                    else:                                # stored or kept: this step's fake is shown
                        assert torch.equal(_bits(rec[shown]), _bits(rec[fake])), f"{what}: {n} was not shown its own fake"
                        if plan == [-2]:
                            slot[r][n] = rec[fake]
                _assert_launches(rec["log"], buckets, "backward" if i > 0 else "start", what)
                assert all(v == v and abs(v) != float("inf") for v in rec["metrics"].values()), (what, rec["metrics"])
            _assert_replicas(recs[0], recs[1], names, f"pool step {i}")
            if i == 1:
                shown_step1 = {shown: torch.cat([recs[0][shown], recs[1][shown]]) for _, _, shown in POOLS}
                two = {k: recs[0][k] for k in ["metrics"] + [f"{n}.flat_grad" for n in names]}
            del recs

        # step 1 against one process at batch 2 whose pools show what the two ranks' pools showed.  The batches of step 0 and
        # step 1 differ, so a rank that showed its discriminator the wrong image is O(1) in that discriminator's fake term
        model = _configured(pkg, arch, device, DP_LR, dict(pool_size=1, pool_seed=0), {})
        model.image_pools = {n: _RecordedPool([None, pkg.ops.to_nhwc(shown_step1[shown].to(device))]) for n, _, shown in POOLS}
        for step in STEPS[:2]:
            _inject_eps(pkg, arch, step)
            m = model.training_step(_batch(pkg, arch, step, device))
        assert all(not p.shown for p in model.image_pools.values())
        assert list(two["metrics"]) == list(m)
        for k, v in m.items():                           # the existing second-step check: 1e-3, near-zero means at the 1e-2 level
            assert abs(two["metrics"][k] - v) <= 1e-3 * max(abs(v), 1e-2), f"pool step 1 {k}: 2 ranks {two['metrics'][k]} vs big batch {v}"
        for name in names:
            err = _grad_distance(two[f"{name}.flat_grad"], getattr(model, name).flat_grad.cpu())
            print(f"pool step 1 {name}: 0.5 x exchanged gradient vs batch 2: {err:.3e} (bound {GRAD_BOUND:g})")
            assert err <= GRAD_BOUND, f"pool step 1 {name}: averaged shard gradients differ from the big-batch gradient by {err:.2e}"
        del model

        # launching the buckets from inside the backward changes no bit: a discriminator bucket reduced before the extra call's
        # weight gradient had landed would
        _run_two_ranks(ref_cfg)
        for i in range(len(STEPS)):
            got, ref = _load(cfg, 0, f"step{i}"), _load(ref_cfg, 0, f"step{i}")
            assert all(w == "start" for *_, w in ref["log"]) and len(ref["log"]) == sum(buckets.values())
            assert got["metrics"] == ref["metrics"], f"pool step {i}: metrics {got['metrics']} vs {ref['metrics']}"
            for name in names:
                for buf in ("flat_grad", "flat_param"):
                    assert torch.equal(_bits(got[f"{name}.{buf}"]), _bits(ref[f"{name}.{buf}"])), \
                        f"pool step {i} {name}.{buf}: launching the buckets from inside the backward changed the result"
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time image_pool: {time.monotonic() - t0:.1f} s")


# ------------------------------------------------------------------ 3. a NaN on one rank
NAN_STEPS = STEPS + (6,)                # healthy, NaN on rank 1, healthy, NaN on rank 1 again


@pytest.mark.parametrize("arch", ["vae", "autoencoder"])
def test_a_nan_on_one_rank_skips_the_step_on_both(arch, pkg, device, tmp_path):
    """Steps 1 and 3: one NaN pixel in rank 1's input.  vae: the NaN reaches rank 0 through the summed gradient, and Adam, the EMA
    launch and both replicas have to agree on the device to write nothing.  autoencoder: the host guard decides through any_rank
    before any gradient exists, and reports the skip from the host.  Feeding a NaN is ordinary arithmetic (the existing poison
    tests).  The second NaN step is there for the average: after step 0 it IS the parameters (the first update copies), so an EMA
    launch that ignored the skip in step 1 would write the bits that are there already; after step 2 it would not."""
    t0 = time.monotonic()
    kept = ("flat_param", "exp_avg", "exp_avg_sq", "flat_ema")
    cfg = _cfg(arch, tmp_path, tag="nan", opt_kw=dict(clip_grad_norm=CLIP[arch], ema_decay=EMA_DECAY), nan_steps=(1, 3),
               steps=NAN_STEPS)
    name = "optimizer"
    try:
        _run_two_ranks(cfg)                              # neither rank hangs: the join limit is the detector
        steps = [[_load(cfg, r, f"step{i}") for r in range(2)] for i in range(len(NAN_STEPS))]
        for r in range(2):
            what = f"{arch} rank {r}"
            for i in (0, 2):                             # the healthy steps
                m = steps[i][r]["metrics"]
                assert m["grad_skipped"] == 0.0 and "nan_detected" not in m, (what, i, m)
                assert all(v == v and abs(v) != float("inf") for v in m.values()), (what, i, m)
                for buf in BUFFERS:
                    assert torch.isfinite(steps[i][r][f"{name}.{buf}"]).all().item(), f"{what}: {name}.{buf} is not finite after step {i}"
            for i in (1, 3):                             # the steps with a NaN on rank 1: nothing is written, on either rank
                before, rec = steps[i - 1][r], steps[i][r]
                for buf in kept:
                    a, b = before[f"{name}.{buf}"], rec[f"{name}.{buf}"]
                    assert torch.equal(_bits(a), _bits(b)), \
                        f"{what}: skipped step {i} wrote {name}.{buf}: {(_bits(a) != _bits(b)).sum().item()} of {a.numel()} elements changed"
                assert rec["metrics"]["grad_skipped"] == 1.0, (what, i, rec["metrics"])
                if arch == "autoencoder":
                    assert rec["metrics"]["nan_detected"] is True and rec["log"] == [], (what, i, rec["metrics"], rec["log"])
                else:
                    assert rec[f"{name}.clip_state"][2].item() == 1.0 and rec["metrics"]["G_loss"] != rec["metrics"]["G_loss"], \
                        (what, i, rec["metrics"])
            for buf in kept:                             # and the healthy step in between trained
                assert not torch.equal(_bits(steps[1][r][f"{name}.{buf}"]), _bits(steps[2][r][f"{name}.{buf}"])), \
                    f"{what}: {name}.{buf} did not move in step 2"
            assert not torch.equal(_bits(steps[2][r][f"{name}.flat_ema"]), _bits(steps[2][r][f"{name}.flat_param"]))
        for i in (0, 2):
            _assert_replicas(steps[i][0], steps[i][1], (name,), f"{arch} NaN run, step {i}")
        for i in (1, 3):                                 # clip_state aside: the host-side skip never touches it
            for buf in kept:
                assert torch.equal(_bits(steps[i][0][f"{name}.{buf}"]), _bits(steps[i][1][f"{name}.{buf}"])), (arch, i, buf)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    print(f"wall time nan[{arch}]: {time.monotonic() - t0:.1f} s")
