"""CPU: host-side logic that needs no GPU — the synthetic generator, layout arithmetic, the CLI surface,
and the data-parallel gradient exchange over gloo with world_size 2."""
import importlib
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_synth_is_deterministic_and_well_distributed(pkg):
    s = pkg.synth
    a = s.normal((4, 3, 16, 16), 7, "w")
    assert np.array_equal(a, s.normal((4, 3, 16, 16), 7, "w"))
    assert not np.array_equal(a, s.normal((4, 3, 16, 16), 8, "w"))
    assert not np.array_equal(a, s.normal((4, 3, 16, 16), 7, "v"))
    big = s.normal((1 << 18,), 1, "moments")
    assert abs(big.mean()) < 1e-2 and abs(big.std() - 1) < 1e-2
    u = s.uniform((1 << 18,), 1, "u")
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 5e-3
    sd = s.state_dict_like({"a.weight": (8, 4, 3, 3), "a.bias": (8,), "h.weight_v": (64,), "h.weight_u": (1,)}, 3)
    assert abs(sd["a.weight"].std() - np.sqrt(2.0 / (8 * 9))) < 0.03
    assert not sd["a.bias"].any()
    assert abs(np.linalg.norm(sd["h.weight_v"]) - 1) < 1e-6 and abs(abs(sd["h.weight_u"][0]) - 1) < 1e-6


def test_nhwc_view_arithmetic(pkg):
    ops = pkg.ops
    assert [ops.pitch(c) for c in (1, 3, 4, 5, 64)] == [4, 4, 4, 8, 64]
    phys = torch.arange(2 * 5 * 7 * 4, dtype=torch.float32).reshape(2, 5, 7, 4)
    v = ops.logical_of(phys, 3)
    assert tuple(v.shape) == (2, 3, 5, 7) and ops.is_nhwc_view(v)
    assert v[1, 2, 3, 4].item() == phys[1, 3, 4, 2].item()
    assert torch.equal(ops.phys_of(v), phys)
    assert not ops.is_nhwc_view(torch.zeros(2, 3, 5, 7))
    x8 = torch.zeros(2, 8, 5, 7).contiguous(memory_format=torch.channels_last)
    assert ops.is_nhwc_view(x8)                                   # torch channels_last IS the layout for C % 4 == 0


def test_state_dict_surface_matches_the_reference(pkg):
    """Key names / shapes the reference's checkpoints carry."""
    m = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False)
    sd = m.state_dict()
    assert tuple(sd["G.encoder.model.1.conv.weight"].shape) == (128, 256, 3, 3)
    assert tuple(sd["DX.model.4.weight_orig"].shape) == (1, 512, 16, 16)
    assert tuple(sd["DX.model.4.weight_u"].shape) == (1,) and tuple(sd["DX.model.4.weight_v"].shape) == (131072,)
    assert tuple(sd["F.variational_encoder_block.logvarConv.1.conv.weight"].shape) == (64, 64, 3, 3)
    assert sum(p.numel() for p in m.parameters()) == 138208008
    assert len(list(m.F.parameters())) + len(list(m.G.parameters())) == 72
    assert len(list(m.DX.parameters())) + len(list(m.DY.parameters())) == 20
    v = pkg.Networks.VariationalAutoencoder(latent_dim=1024)
    assert sum(p.numel() for p in v.parameters()) == 102161667
    for cls in ("CaSb", "D", "R", "U", "S", "L", "Encoder", "Decoder", "VariationalEncoderBlock",
                "VariationalDecoderBlock", "Discriminator", "Autoencoder", "VariationalAutoencoder", "CycleVAEGAN"):
        assert hasattr(pkg.Networks, cls)
    for name in ("forward", "configure_optimizers", "save_optimizer_states", "load_optimizer_states",
                 "configure_loss", "training_step", "validation_step"):
        assert callable(getattr(pkg.Networks.CycleVAEGAN, name))
        assert callable(getattr(pkg.Networks.CycleAEGAN, name))
    # CycleAEGAN (reference Networks.py:1618-1636): two plain autoencoders + two discriminators, no VAE block.  The
    # golden arrays of the reference's own step name every state_dict entry (ck.<name>)
    a = pkg.Networks.CycleAEGAN(paired=False)
    names = {k.split("/ck.", 1)[1] for k in np.load(os.path.join(ROOT, "tests", "golden", "cycleaegan.npz")).files
             if k.startswith("cag256_unpaired@step1/ck.")}
    assert set(a.state_dict()) == names
    assert not any("variational" in k for k in a.state_dict())
    assert sum(p.numel() for p in a.parameters()) == 2 * (43955328 + 20453507) + 2 * 2887617


def test_cli_keeps_the_reference_flags_and_defaults():
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")
    a = train.build_parser().parse_args([])
    ref_defaults = dict(architecture="autoencoder", paired=False, pretrained_doubleae=None, pretrained_doublevae=None,
                        data_dir="dataset", source_modality=None, target_modality=None, image_size=256, test_split=0.1,
                        dataset="hypersim", batch_size=5, epochs=100, lr=0.0002, lambda_kl=1e-5, lambda_gan=1.0,
                        lambda_identity=5.0, lambda_cycle=10.0, lambda_recon=1.0, output_dir="runs", save_freq=10,
                        log_image_freq=5, resume=None, num_workers=1, no_cuda=False)
    for k, v in ref_defaults.items():
        assert getattr(a, k) == v, k
    assert a.latent_dim == 64
    b = train.build_parser().parse_args(["--architecture", "vae_cyclegan", "--dataset", "synthetic", "--paired", "--latent_dim", "1024"])
    assert train.ALIASES[b.architecture] == "cyclevaegan" and b.paired and b.latent_dim == 1024
    assert isinstance(train.create_model("ae"), importlib.import_module("vae-cyclegan-implementation_amd").Networks.Autoencoder)
    with pytest.raises(ValueError):
        train.create_model("nonsense")
    assert set(train.BUILT) == set(train.REFERENCE_ARCHS)          # every architecture of the reference's factory is built
    N = importlib.import_module("vae-cyclegan-implementation_amd").Networks
    assert type(train.create_model("doubleae")) is N.DoubleAutoencoder and type(train.create_model("doublevae")) is N.DoubleVariationalAutoencoder
    assert type(train.create_model("aegan")) is N.AEGAN and type(train.create_model("vaegan")) is N.VAEGAN
    for arch, cls in (("cycleae", N.CycleAE), ("cyclevae", N.CycleVAE), ("cycleaegan", N.CycleAEGAN), ("cyclevaegan", N.CycleVAEGAN)):
        assert type(train.create_model(arch, paired=False)) is cls


def test_train_epoch_averages_like_the_reference():
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")

    class Fake:
        def __init__(self):
            self.i = 0

        def train(self):
            pass

        def training_step(self, batch):
            self.i += 1
            return {"G_loss": float(self.i), "other": 10.0 * self.i}
    batches = [{"x": torch.zeros(1), "y": torch.zeros(1)} for _ in range(3)]
    avg, comps, out, lx, ly = train.train_epoch(Fake(), batches, "cpu", type("A", (), {})())
    assert avg == 2.0 and comps == {"G_loss": 2.0, "other": 20.0} and out is None and lx is batches[-1]["x"]


def test_validate_averages_like_the_reference():
    """reference train.py:131-171: eval mode, Gx / Fy popped before the averaging, G_loss the headline."""
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")

    class Fake:
        def __init__(self):
            self.i, self.mode = 0, None

        def eval(self):
            self.mode = "eval"

        def validation_step(self, batch):
            assert self.mode == "eval" and not torch.is_grad_enabled()
            self.i += 1
            return {"G_loss": float(self.i), "loss_kl": 4.0 * self.i, "Gx": torch.full((1,), float(self.i)), "Fy": torch.zeros(1)}
    batches = [{"x": torch.zeros(1), "y": torch.ones(1)} for _ in range(4)]
    avg, comps, gx, fy, lx, ly = train.validate(Fake(), batches, "cpu", type("A", (), {})())
    assert avg == 2.5 and comps == {"G_loss": 2.5, "loss_kl": 10.0}
    assert gx.item() == 4.0 and fy is not None and lx is batches[-1]["x"] and ly is batches[-1]["y"]


def test_checkpoint_skeleton_fixture_matches_our_state_dict_surface(pkg):
    """tests/golden/checkpoint_skeleton.json (structure of checkpoints written by the reference's utils.save_checkpoint):
    the model_state_dict section names exactly our modules' state_dict entries, with the same shapes."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "checkpoint_skeleton.json")) as fh:
        skel = json.load(fh)
    for arch, ctor in (("autoencoder", pkg.Networks.Autoencoder), ("vae", lambda: pkg.Networks.VariationalAutoencoder(64)),
                       ("cyclevaegan", lambda: pkg.Networks.CycleVAEGAN(64, False))):
        assert list(skel[arch]) == ["epoch", "model_state_dict", "optimizer_states", "loss", "args"]
        ours = {k: list(v.shape) for k, v in ctor().state_dict().items()}
        ref = {k: v["tensor"] for k, v in skel[arch]["model_state_dict"].items()}
        assert list(ours) == list(ref) and ours == ref
        for name, opt in skel[arch]["optimizer_states"].items():
            assert name in ("optimizer", "optimizer_G", "optimizer_D")
            assert set(opt) == {"state", "param_groups"} and len(opt["param_groups"]) == 1


def test_pretrained_double_checkpoints_map_onto_cycle_models(pkg, tmp_path):
    """reference utils.py:57-239: a DoubleAE / DoubleVAE checkpoint initialises the generators of a Cycle model —
    G (A->B) from the encoder and the B side, F (B->A) from the encoder and the A side.  Pure state_dict work (no GPU)."""
    N, utils = pkg.Networks, pkg.utils
    torch.manual_seed(3)
    d = N.DoubleVariationalAutoencoder(latent_dim=64)
    with torch.no_grad():
        for i, p in enumerate(d.parameters()):          # distinguishable values everywhere (biases are zero at init)
            p.add_(0.001 * (i + 1))
    fn = str(tmp_path / "dvae.pth")
    torch.save({"epoch": 0, "model_state_dict": d.state_dict(), "loss": 0.0, "args": {}}, fn)
    for cyc in (N.CycleVAE(latent_dim=64, paired=False), N.CycleVAEGAN(latent_dim=64, paired=False)):
        utils.load_pretrained_doublevae_to_cyclevae(cyc, fn, "cpu")
        sd, cs = d.state_dict(), cyc.state_dict()
        for k, v in sd.items():
            head, rest = k.split(".", 1)
            targets = {"encoder": ("G.encoder.", "F.encoder."), "decoder_A": ("F.decoder.",), "decoder_B": ("G.decoder.",),
                       "vae_encoder_block_A": ("F.variational_encoder_block.",), "vae_encoder_block_B": ("G.variational_encoder_block.",),
                       "vae_decoder_block_A": ("F.variational_decoder_block.",), "vae_decoder_block_B": ("G.variational_decoder_block.",)}[head]
            for t in targets:
                assert torch.equal(cs[t + rest], v), (k, t)
    a = N.DoubleAutoencoder()
    with torch.no_grad():
        for i, p in enumerate(a.parameters()):
            p.add_(0.001 * (i + 1))
    fn = str(tmp_path / "dae.pth")
    torch.save({"epoch": 0, "model_state_dict": a.state_dict(), "loss": 0.0, "args": {}}, fn)
    for cyc in (N.CycleAE(paired=False), N.CycleAEGAN(paired=False)):
        utils.load_pretrained_doubleae_to_cycleae(cyc, fn, "cpu")
        sd, cs = a.state_dict(), cyc.state_dict()
        assert torch.equal(cs["G.decoder.model.5.conv.bias"], sd["decoder_B.model.5.conv.bias"])
        assert torch.equal(cs["F.decoder.model.5.conv.bias"], sd["decoder_A.model.5.conv.bias"])
        assert torch.equal(cs["G.encoder.model.2.conv.weight"], sd["encoder.model.2.conv.weight"])
        assert torch.equal(cs["F.encoder.model.2.conv.weight"], sd["encoder.model.2.conv.weight"])
    with pytest.raises(FileNotFoundError):
        utils.load_pretrained_doubleae_to_cycleae(N.CycleAE(), str(tmp_path / "none.pth"), "cpu")


# ------------------------------------------------------------------ data parallel over gloo, world_size 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    torch.set_num_threads(2)
    pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    oracle = importlib.import_module("vcg_oracle")
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    try:
        # a small generator-shaped model: the VAE bottleneck + one residual block, evaluated by the oracle
        shapes = {"variational_encoder_block.muConv.conv.weight": (8, 16, 3, 3), "variational_encoder_block.muConv.conv.bias": (8,),
                  "variational_encoder_block.logvarConv.0.conv.weight": (8, 16, 3, 3), "variational_encoder_block.logvarConv.0.conv.bias": (8,),
                  "variational_encoder_block.logvarConv.1.conv.weight": (8, 8, 3, 3), "variational_encoder_block.logvarConv.1.conv.bias": (8,),
                  "r.conv1.weight": (16, 16, 3, 3), "r.conv1.bias": (16,), "r.conv2.weight": (16, 16, 3, 3), "r.conv2.bias": (16,)}
        P = {k: torch.from_numpy(v) for k, v in pkg.synth.state_dict_like(shapes, 11, bias_std=0.05).items()}
        names = list(P)
        B = 4                                   # global batch; each rank takes B/world samples
        x = torch.from_numpy(pkg.synth.normal((B, 16, 6, 6), 11, "dp/x"))
        eps = torch.from_numpy(pkg.synth.normal((B, 8, 6, 6), 11, "dp/eps"))

        def loss_and_grads(xs, es):
            Q = {k: v.clone().requires_grad_(True) for k, v in P.items()}
            h = oracle.r_block(xs, Q, "r.")
            z, mu, lv = oracle.variational_encoder_block(h, Q, "variational_encoder_block.", es)
            loss = oracle.l1(z, torch.zeros_like(z)) + 1e-3 * oracle.kl_loss(mu, lv)
            gs = torch.autograd.grad(loss, [Q[n] for n in names])
            return loss.detach(), torch.cat([g.reshape(-1) for g in gs])

        lo = rank * (B // world)
        loss, flat = loss_and_grads(x[lo:lo + B // world], eps[lo:lo + B // world])

        class Opt:                               # what GradReducer needs from optim.FusedAdam
            pass
        opt = Opt()
        opt.flat_grad, opt.grad_scale = flat.clone(), 1.0
        red = pkg.parallel.GradReducer(bucket_bytes=4096)     # several buckets
        red.start(opt)
        red.finish(opt)
        avg = opt.flat_grad * opt.grad_scale
        full_loss, full = loss_and_grads(x, eps)              # the single-process big-batch gradient
        err = ((avg - full).norm() / full.norm()).item()
        m = red.average_metrics(loss.reshape(1).clone())
        merr = abs(m.item() - full_loss.item()) / abs(full_loss.item())
        # identical replicas after broadcast
        lin = torch.nn.Linear(3, 2)
        with torch.no_grad():
            lin.weight.fill_(float(rank + 1))
        pkg.parallel.broadcast_parameters(lin)
        q.put((rank, err, merr, opt.grad_scale, lin.weight.detach().flatten()[0].item()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_gradient_exchange_equals_big_batch_gradient():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, err, merr, scale, w0 in res:
        assert err < 1e-5, f"rank {rank}: averaged shard gradients differ from the big-batch gradient by {err:.2e}"
        assert merr < 1e-5
        assert scale == 0.5 and w0 == 1.0


def _bucket_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    try:
        # what GradReducer needs from optim.FusedAdam: params, offsets, flat_grad (+ grad_scale, which it sets)
        class Opt:
            def __init__(self, sizes, tag):
                self.params = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
                self.offsets, off = [], 0
                for n in sizes:
                    self.offsets.append(off)
                    off += (n + 3) // 4 * 4
                self.flat_grad = torch.zeros(off)
                self.grad_scale, self.tag = 1.0, tag
        # "generator": 6 conv layers as (weight, bias) pairs in forward order; layers 0-2 are used by TWO forwards of the step
        sizes = [4000, 40, 3000, 30, 5000, 50, 2000, 20, 6000, 60, 1000, 10]
        optG = Opt(sizes, "optimizer_G")
        optD = Opt([800, 8], "optimizer_D")
        red = pkg.parallel.GradReducer(bucket_bytes=4 * 6000)      # buckets close once they hold >= 6000 floats
        uses = [2, 2, 2, 1, 1, 1]

        def backward(step):
            """reverse layer order, like autograd; each report ADDS that use's gradient (the kernels accumulate)"""
            for use in (0, 1):
                for layer in reversed(range(6)):
                    if uses[layer] <= use:
                        continue
                    w, b = optG.params[2 * layer], optG.params[2 * layer + 1]
                    for prm, o in ((w, optG.offsets[2 * layer]), (b, optG.offsets[2 * layer + 1])):
                        optG.flat_grad[o:o + prm.numel()] += (rank + 1) * (layer + 1) * (step + 1)
                    # layer 0's gradients come from the "main" stream, everything else from the "side" stream (the tokens stand
                    # for HIP streams: on the CPU only the ordering decisions are recorded, parallel.GradReducer._order_after)
                    red.note(w, b, "main" if layer == 0 else "side")
                    red.note(optD.params[0], optD.params[1], "side")    # by-product reports on ANOTHER optimizer's parameters
        logs = []
        for step in range(3):
            optG.flat_grad.zero_()
            optD.flat_grad.fill_(7.0 + rank)                            # must never be touched by the G phase
            n0 = len(red.log)
            red.begin(optG)
            backward(step)
            red.start(optG)
            red.finish(optG)
            logs.append(red.log[n0:])
            want = torch.zeros_like(optG.flat_grad)
            for layer in range(6):
                for j in (0, 1):
                    o, n = optG.offsets[2 * layer + j], optG.params[2 * layer + j].numel()
                    want[o:o + n] = sum(r + 1 for r in range(world)) * (layer + 1) * (step + 1) * uses[layer]
            assert torch.equal(optG.flat_grad, want), f"step {step}: reduced gradient is wrong"
            assert torch.equal(optD.flat_grad, torch.full_like(optD.flat_grad, 7.0 + rank)), "D's by-product gradients were reduced"
            assert optG.grad_scale == 1.0 / world and optG._exchange_pending is False
        plan = red._plans[id(optG)]
        # a report on a bucket that is already in flight is an error, not a silent race
        red.begin(optG)
        backward(9)
        try:
            red.note(optG.params[10], optG.params[11], None)
            raised = False
        except RuntimeError:
            raised = True
        red.start(optG)
        red.finish(optG)
        flag_any = red.any_rank(rank == 1)
        flag_none = red.any_rank(False)
        q.put((rank, logs, list(plan.buckets), raised, flag_any, flag_none, list(red.wait_log), dict(plan.bucket_of), [id(p) for p in optG.params]))
    finally:
        dist.destroy_process_group()


def test_buckets_are_exchanged_from_inside_the_backward_in_completion_order():
    """parallel.GradReducer: the first backward learns how often each parameter reports; from the second on a bucket is
    all-reduced the moment its last report arrives — later layers first, layers shared by two forwards last — the sum is
    the all-rank sum, parameters of another optimizer are never reduced, and a late report on a launched bucket raises."""
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bucket_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, logs, buckets, raised, flag_any, flag_none, waits, bucket_of, pids in res:
        assert len(buckets) >= 3 and buckets[0][0] == 0 and all(a[1] == b[0] for a, b in zip(buckets, buckets[1:]))
        first, second, third = logs
        assert [w for *_, w in first] == ["start"] * len(buckets)            # learning step: everything after the backward
        assert [b for _, b, *_ in first] == list(range(len(buckets)))
        for log in (second, third):
            assert sorted(b for _, b, *_ in log) == list(range(len(buckets)))   # every bucket exactly once
            assert all(w == "backward" for *_, w in log), log                    # ... and from inside the backward
            order = [b for _, b, *_ in log]
            assert order == sorted(order, reverse=True), f"buckets should complete from the last layers to the first: {order}"
            assert all(tag == "optimizer_G" for tag, *_ in log)
        assert raised and flag_any is True and flag_none is False
        # ADVICE r2 / VERDICT r2 #6a: bucket 0 holds layer 0 (reported from "main", LAST) and layer 1 (reported from "side"):
        # its collective is launched on "main" and must first be ordered after "side"; the buckets whose reports all came
        # from "side" wait for nobody
        b0 = bucket_of[pids[0]]
        assert bucket_of[pids[2]] == b0, "the test's bucket 0 should hold layers 0 and 1"
        w0 = [(st, others) for b, st, others in waits if b == b0]
        assert w0 and all(st == "main" and others == ["side"] for st, others in w0), w0
        assert all(others == [] for b, st, others in waits if b != b0 and st == "side")


def _nan_vote_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    N = pkg.Networks
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    try:
        # Autoencoder.training_step itself (the unbound function), on a stand-in whose forward / loss / optimizer are CPU
        # torch: the guard, the collective vote, begin / start / finish and the metric averaging are the real code
        class Opt:
            def __init__(self, params):
                self.params = list(params)
                self.offsets, off = [], 0
                for p in self.params:
                    self.offsets.append(off)
                    off += p.numel()
                self.flat_grad = torch.zeros(off)
                for p, o in zip(self.params, self.offsets):
                    p.grad = self.flat_grad[o:o + p.numel()].view(p.shape)
                self.grad_scale, self.steps_taken, self.zeroed = 1.0, 0, 0

            def zero_grad(self):
                self.flat_grad.zero_()
                self.zeroed += 1

            def step(self):
                self.steps_taken += 1
                with torch.no_grad():
                    for p, o in zip(self.params, self.offsets):
                        p -= 0.1 * self.grad_scale * self.flat_grad[o:o + p.numel()].view(p.shape)

        class Stub:
            def __init__(self):
                torch.manual_seed(0)
                self.lin = torch.nn.Linear(4, 4)
                self.optimizer = Opt(self.lin.parameters())
                self.grad_reducer = pkg.parallel.GradReducer(bucket_bytes=16)
                self.poison = False
                self.loss_fn = lambda out, y: (out - y).abs().mean() * (float("nan") if self.poison else 1.0)

            def __call__(self, x):
                return self.lin(x)
        orig = pkg.ops.to_nhwc
        pkg.ops.to_nhwc = lambda t: t
        try:
            st = Stub()
            x = torch.full((2, 4), float(rank + 1))
            y = torch.zeros(2, 4)
            st.poison = rank == 1                                   # step 1: a NaN loss on rank 1 ONLY
            m1 = N.Autoencoder.training_step(st, {"x": x, "y": y})
            taken1 = st.optimizer.steps_taken
            st.poison = False                                       # step 2: healthy everywhere -> both ranks exchange and step
            w_before = st.lin.weight.detach().clone()
            m2 = N.Autoencoder.training_step(st, {"x": x, "y": y})
            q.put((rank, bool(m1.get("nan_detected")), taken1, st.optimizer.steps_taken, m2["G_loss"],
                   st.lin.weight.detach().clone(), float((st.lin.weight.detach() - w_before).abs().max())))
        finally:
            pkg.ops.to_nhwc = orig
    finally:
        dist.destroy_process_group()


def test_nan_on_one_rank_makes_both_ranks_skip_and_neither_hangs():
    """VERDICT r2 weak #1d / ADVICE r1: two real ranks (gloo), a NaN loss injected on rank 1 only.  Both ranks must take the
    skip branch of Autoencoder.training_step (reference Networks.py:357-372) — rank 0, whose loss is finite, included — and
    neither may enter the gradient exchange alone (the q.get timeout below is the hang detector).  The next, healthy step
    runs the exchange on both and leaves identical replicas with the rank-averaged loss logged."""
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_nan_vote_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, skipped, taken1, taken2, loss2, w, moved in res:
        assert skipped, f"rank {rank} did not skip the step in which rank 1 saw a NaN"
        assert taken1 == 0 and taken2 == 1 and moved > 0
    assert torch.equal(res[0][5], res[1][5]), "replicas diverged after the healthy step"
    assert res[0][4] == res[1][4] and res[0][4] == res[0][4]        # the same, finite, rank-averaged loss on both


def _resume_seed_worker(rank, world, port, path, q):
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    try:
        import argparse

        class Tiny(torch.nn.Module):                               # what utils.save / load_checkpoint need of a model
            def __init__(self):
                super().__init__()
                self.lin = torch.nn.Linear(2, 2)
                self.optimizer = object()

            def save_optimizer_states(self):
                return {"optimizer": {"state": {}, "param_groups": []}}

            def load_optimizer_states(self, states):
                assert "optimizer" in states
        model = Tiny()
        base = 1234
        pkg.ops.manual_seed(pkg.ops.rank_seed(base, rank))        # what train.main does
        pkg.ops._RNG["offset"] = 4242                              # ... and some steps later
        mine = dict(pkg.ops._RNG)
        if rank == 0:                                              # only rank 0 writes (train.py)
            pkg.utils.save_checkpoint(model, 3, 0.5, argparse.Namespace(seed=base), path)
        dist.barrier()
        pkg.ops.manual_seed(999)                                   # a fresh process: then --resume
        pkg.utils.load_checkpoint(model, path, torch.device("cpu"))
        q.put((rank, mine, dict(pkg.ops._RNG)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_resume_restores_each_ranks_own_eps_stream(tmp_path):
    """rank 0 writes the checkpoint; on --resume every rank must continue ITS eps stream — the
    per-rank seed re-derived from the saved base — not rank 0's (all shards of the global batch would draw the same noise)."""
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    path = str(tmp_path / "ck.pth")
    procs = [ctx.Process(target=_resume_seed_worker, args=(r, world, port, path, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, before, after in res:
        assert after == before, f"rank {rank}: resumed eps stream {after} != the stream it had {before}"
    assert res[0][2]["seed"] != res[1][2]["seed"] and res[0][2]["offset"] == res[1][2]["offset"] == 4242
    # a round-2 file (no base_seed, written by rank 0) still restores rank 0's stream exactly
    ck = torch.load(path, weights_only=False)
    assert ck["vcg_eps_rng"]["rank"] == 0 and ck["vcg_eps_rng"]["base_seed"] == 1234


def test_autoencoder_nan_guard_is_collective_under_data_parallelism():
    """the NaN / Inf early return of Autoencoder.training_step (reference Networks.py:357-372) must be decided by
    all ranks together, before anyone enters the gradient exchange, and the logged loss must be the rank average."""
    import ast
    import inspect
    N = importlib.import_module("vae-cyclegan-implementation_amd").Networks
    src = inspect.getsource(N.Autoencoder.training_step)
    tree = ast.parse("class _:\n" + src if src.startswith("    ") else src)
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, (ast.Attribute, ast.Name))]
    name = lambda c: c.func.attr if isinstance(c.func, ast.Attribute) else c.func.id   # noqa: E731
    order = [name(c) for c in sorted(calls, key=lambda c: (c.lineno, c.col_offset))]
    assert "any_rank" in order and "_backward_and_step" in order
    assert order.index("any_rank") < order.index("_backward_and_step")
    assert "_metrics_to_host" in order


def test_bench_extra_steps_are_entered_by_every_rank():
    """bench.py's roofline pass runs two extra training steps; with N > 1 each contains the gradient all-reduce, so the
    call must not sit behind a rank test (rank 0 alone in a collective hangs the job: seen on a 2-rank rehearsal)."""
    import ast
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)

    def mentions_rank(node):
        return any(isinstance(n, ast.Name) and n.id == "rank" for n in ast.walk(node))

    class V(ast.NodeVisitor):
        def __init__(self):
            self.guards, self.bad, self.seen = [], [], 0

        def visit_If(self, node):
            self.guards.append(mentions_rank(node.test))
            for b in node.body:
                self.visit(b)
            self.guards.pop()
            for b in node.orelse:
                self.visit(b)

        def visit_Call(self, node):
            if isinstance(node.func, ast.Name) and node.func.id == "measure_roofline":
                self.seen += 1
                if any(self.guards):
                    self.bad.append(node.lineno)
            self.generic_visit(node)

    v = V()
    v.visit(tree)
    assert v.seen == 1 and not v.bad, f"measure_roofline is called under a rank test at bench.py:{v.bad}"


def _bench_module():
    """bench.py as a module; the environment defaults it sets on import are undone (this process may use the GPU later)."""
    import importlib.util
    saved = dict(os.environ)
    try:
        spec = importlib.util.spec_from_file_location("vcg_bench", os.path.join(ROOT, "bench.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.environ.clear()
        os.environ.update(saved)
    return mod


def test_bench_dump_outputs_is_bounded_and_repeatable(tmp_path):
    """bench.py --dump-outputs: one float64 file per metric, one float32 file per state tensor — whole when small, else a sample
    at fixed indices (the same in every run, so two builds can be compared element for element) — within the size budget."""
    bench = _bench_module()
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(300, 400), torch.nn.Linear(400, 5))     # weight 0: 120 000 > DUMP_SAMPLE elements
    with torch.no_grad():
        model[0].weight.copy_(torch.arange(120000, dtype=torch.float32).reshape(400, 300))     # each element holds its flat index
    metrics = {"G_loss": 1.25, "D_loss": 0.5}
    bench.dump_outputs(str(tmp_path / "a"), metrics, model)
    bench.dump_outputs(str(tmp_path / "b"), metrics, model)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert names == sorted([f"metric.{k}.npy" for k in metrics] + [f"param.{k}.npy" for k in model.state_dict()])
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == (np.float64 if n.startswith("metric.") else np.float32) and np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "metric.G_loss.npy") == 1.25
    got = np.load(tmp_path / "a" / "param.0.weight.npy")         # = the sampled indices: distinct, ascending, in range
    assert got.size == bench.DUMP_SAMPLE and (np.diff(got) > 0).all() and got[0] >= 0 and got[-1] < 120000
    assert np.array_equal(np.load(tmp_path / "a" / "param.1.weight.npy"), model.state_dict()["1.weight"].reshape(-1).numpy())
    # many tensors: each one's share of the budget shrinks, the total stays under it
    many = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(5000)) for _ in range(64)])
    bench.DUMP_BUDGET_BYTES = 1 << 18
    bench.dump_outputs(str(tmp_path / "c"), metrics, many)
    total = sum(np.load(tmp_path / "c" / n).nbytes for n in os.listdir(tmp_path / "c"))
    assert total <= bench.DUMP_BUDGET_BYTES + 8 * len(metrics), total


def _validate_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    train = importlib.import_module("vae-cyclegan-implementation_amd.train")
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    try:
        class Fake:
            grad_reducer = pkg.parallel.GradReducer()

            def eval(self):
                pass

            def validation_step(self, batch):
                v = float(batch["x"].item())
                return {"G_loss": v, "loss_kl": 2.0 * v, "Gx": batch["x"], "Fy": batch["y"]}
        # 3 test batches over 2 ranks: rank 0 sees values 1, 3; rank 1 sees 2 — then a set smaller than the world: rank 1 sees nothing
        out = []
        for values in ([1.0, 2.0, 3.0], [5.0]):
            mine = [{"x": torch.tensor([v]), "y": torch.zeros(1)} for v in values[rank::world]]
            avg, comps, *_ = train.validate(Fake(), mine, "cpu", type("A", (), {})())
            out.append((avg, comps))
        q.put((rank, out))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_validate_pools_uneven_and_empty_shards_across_ranks():
    """under data parallelism `validate` used to average per-rank means (wrong for uneven shards) and divided by zero
    on a rank whose shard of a tiny test split was empty.  Two gloo ranks: the result is the batch-weighted mean over ALL batches,
    identical on both ranks, and an empty shard neither crashes nor hangs the collective."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_validate_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank in range(world):
        (a1, c1), (a2, c2) = res[rank]
        assert a1 == 2.0 and c1 == {"G_loss": 2.0, "loss_kl": 4.0}, (rank, a1, c1)
        assert a2 == 5.0 and c2 == {"G_loss": 5.0, "loss_kl": 10.0}, (rank, a2, c2)


# ------------------------------------------------------------------ SURVEY.md §8e's own DDP fixture: the reference at batch 8 vs 8 ranks x batch 1
def _dp8_worker(rank, world, port, pfile, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    torch.set_num_threads(1)
    pkg = importlib.import_module("vae-cyclegan-implementation_amd")
    oracle = importlib.import_module("vcg_oracle")
    from cases import LAMBDAS, LR, SEED
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    try:
        raw = np.load(pfile, mmap_mode="r")
        P = {k[len("cvg256_b8."):]: torch.from_numpy(np.array(raw[k])) for k in raw.files}
        x, y = pkg.synth.batch(world, 256, SEED, step=0)
        eps = pkg.synth.eps_list(6, (world, 64, 16, 16), SEED, step=0)
        sl = slice(rank, rank + 1)
        m, _, g_grads, d_grads = oracle.cyclevaegan_step(P, {}, torch.from_numpy(x[sl]), torch.from_numpy(y[sl]),
                                                         [torch.from_numpy(e[sl]) for e in eps], LR, False,
                                                         lambda_cycle=LAMBDAS["lambda_cycle"], lambda_gan=LAMBDAS["lambda_gan"],
                                                         lambda_kl=LAMBDAS["lambda_kl"], lambda_identity=LAMBDAS["lambda_identity"])
        red = pkg.parallel.GradReducer(bucket_bytes=64 << 20)
        out = {}
        for tag, grads in (("G", g_grads), ("D", d_grads)):
            names = list(grads)
            # optim.FusedAdam's layout: parameter order, every view 4-element aligned
            offs, off = [], 0
            for n_ in names:
                offs.append(off)
                off += (grads[n_].numel() + 3) // 4 * 4
            flat = torch.zeros(off)
            for n_, o in zip(names, offs):
                flat[o:o + grads[n_].numel()] = grads[n_].reshape(-1)

            class Opt:
                pass
            opt = Opt()
            opt.flat_grad, opt.grad_scale = flat, 1.0
            red.start(opt)
            red.finish(opt)
            assert opt.grad_scale == 1.0 / world
            if rank == 0:
                avg = opt.flat_grad * opt.grad_scale
                out[tag] = {n_: avg[o:o + grads[n_].numel()].view(grads[n_].shape).clone() for n_, o in zip(names, offs)}
        keys = list(m)
        mv = red.average_metrics(torch.tensor([m[k] for k in keys], dtype=torch.float32))
        if rank == 0:
            from conftest import checksum
            cks = {n_: checksum(g) for tag in out for n_, g in out[tag].items()}
            q.put((dict(zip(keys, mv.tolist())), cks))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_eight_ranks_of_batch_one_equal_the_reference_at_batch_eight(pkg, tmp_path):
    """"DDP parity fixture: reference CPU at B=8 vs 8 ranks x B=1".  Eight gloo ranks each evaluate ONE image
    pair of the headline batch (the oracle's restatement of /root/reference/Networks.py:1973-2078, 256 x 256, the fixture's
    parameters and eps), their flat gradients go through parallel.GradReducer (sum-all-reduce of contiguous slices, 1/world in
    grad_scale) and the world-averaged gradient is held to the REFERENCE's batch-8 step (tests/golden/headline.*: fp32 and
    fp64 gradient checksums), the rank-averaged metrics to its metric dict.  ~3 minutes of CPU: the only 8-rank run this
    container can make."""
    import json
    from conftest import GOLDEN, assert_grad_checksum, in_cancelled_bias
    from cases import STEP_BIAS_STD
    world = 8
    arrays = dict(np.load(os.path.join(GOLDEN, "headline.npz")))
    with open(os.path.join(GOLDEN, "headline_meta.json")) as f:
        ref_m = json.load(f)["cvg256_b8"][0]
    model = pkg.Networks.CycleVAEGAN(latent_dim=64, paired=False)
    shapes = {"cvg256_b8." + k: tuple(v.shape) for k, v in model.state_dict().items()}
    del model
    sd = pkg.synth.state_dict_like(shapes, 20261003, bias_std=STEP_BIAS_STD)
    pfile = str(tmp_path / "params.npz")
    np.savez(pfile, **sd)
    del sd
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp8_worker, args=(r, world, port, pfile, q)) for r in range(world)]
    for p in procs:
        p.start()
    metrics, cks = q.get(timeout=1500)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for k, v in ref_m.items():
        assert abs(metrics[k] - v) <= 1e-3 * max(abs(v), 1e-6), f"{k}: 8 ranks {metrics[k]!r}, reference at batch 8 {v!r}"
    bad, seen = [], 0
    for n_, got in cks.items():
        if in_cancelled_bias(n_) or f"cvg256_b8@step1/gck64.{n_}" not in arrays:
            continue
        if n_.endswith("model.4.weight_orig"):
            # the spectral-normed 1 x 131072 weight: its gradient is what is left of G after projecting out W (W / sigma does not
            # depend on |W|), and a BATCH-1 evaluation of it in fp32 on the CPU is rounding noise — measured with the oracle's
            # discriminator: in float64 the batch-2 gradient equals the mean of the two batch-1 gradients to 3e-15, in fp32 they
            # differ by 0.78; the reference's own fp32 run of the batch-1 fixture sits 0.77 from its fp64 run on this tensor
            # (tests/golden/make_golden.py, gen_steps_fp64), at batch 8 only 1e-5.  Eight fp32 batch-1 CPU evaluations are
            # therefore no comparator for it; the GPU test at batch 8 (tests/test_gpu_headline.py) holds it to the fixture.
            continue
        seen += 1
        try:
            assert_grad_checksum(None, arrays[f"cvg256_b8@step1/gck.{n_}"], arrays[f"cvg256_b8@step1/gck64.{n_}"], "grad " + n_,
                                 got=got, key="dp8_batch1")
        except AssertionError as e:
            bad.append(str(e))
    assert seen >= 78 and not bad, f"{len(bad)} of {seen} world-averaged gradients off the reference's batch-8 step:\n" + "\n".join(b[:300] for b in bad[:8])


# ------------------------------------------------------------------ eps draws reserved ahead of time (two directions on two streams)
def test_eps_tickets_keep_the_reference_draw_order(pkg):
    """ops.eps_tickets / use_ticket (Networks.CycleVAEGAN._forward_two_streams): the two translation directions are issued
    interleaved, G(x), F(y), F(G(x)), G(F(y)), but every reparameterisation must draw what it draws in the reference's call order
    G(x), [G(y)], F(G(x)), F(y), [F(x)], G(F(y)) (/root/reference/Networks.py:1997-2006) — injected tensors (parity runs) and
    positions of the on-device Philox stream alike; skipped forwards still consume theirs."""
    ops = pkg.ops
    shp = (2, 64, 4, 4)
    n4 = (2 * 64 * 4 * 4 + 3) // 4
    plan = [(shp, False), (shp, True), (shp, False), (shp, False), (shp, True), (shp, False)]
    # injected mode: the queue holds six tensors in the reference's order
    inj = [torch.full(shp, float(i)) for i in range(6)]
    ops.inject_eps(list(inj))
    tk = ops.eps_tickets(plan, torch.device("cpu"))
    assert tk[1] is None and tk[4] is None and not ops._EPS_QUEUE
    assert [float(tk[i][1].flatten()[0]) for i in (0, 2, 3, 5)] == [0.0, 2.0, 3.0, 5.0]
    # RNG mode: positions are reserved in plan order, whatever order they are used in
    ops.manual_seed(77)
    tk = ops.eps_tickets(plan, torch.device("cpu"))
    assert [tk[i] for i in (0, 2, 3, 5)] == [("offset", 0), ("offset", 2 * n4), ("offset", 3 * n4), ("offset", 5 * n4)]
    assert ops._RNG["offset"] == 6 * n4
    order = []
    for i in (0, 3, 2, 5):                       # the issue order of the two-stream forward
        with ops.use_ticket(tk[i]):
            assert ops.next_eps(shp, torch.device("cpu")) is None      # "draw on device" ...
            order.append(ops._FORCED_OFFSETS.pop(0))                   # ... at the reserved position (what _ReparamFn.forward pops)
    assert order == [0, 3 * n4, 2 * n4, 5 * n4] and not ops._TICKETS
    # a block that runs no reparameterisation leaves its ticket unconsumed: that is an error, not a silent shift of the stream
    with pytest.raises(RuntimeError, match="not consumed"):
        with ops.use_ticket(("offset", 123)):
            pass
    assert not ops._TICKETS
    ops.manual_seed(0)


def test_operand_range_cases_reach_every_fp16_family():
    """tests/test_gpu_operand_range.py runs tiered operands through one case per fp16 x 2 kernel family, picked by the dispatch mirror
    (the smallest reduction length that conv_plan maps to the family): the pick must keep covering every member of FP16_FWD and
    FP16_DGRAD, the thin-fold MFMA kernel, the three Winograd GEMMs and the fp16 weight-gradient branches, one of them from
    `saved` — a plan change that empties a family fails here, naming it."""
    from test_gpu_conv_plans import FP16_DGRAD, FP16_FWD
    from test_gpu_operand_range import TIER_CASES, TIER_REQUIRED, tier_selection
    for b in FP16_FWD:
        assert any(r.startswith(f"fwd {b}") for r in TIER_REQUIRED), b
    for b in FP16_DGRAD:
        assert f"dgrad {b}" in TIER_REQUIRED, b
    sel = tier_selection(TIER_CASES)
    missing = [f for f in TIER_REQUIRED if f not in sel]
    assert not missing, f"no tiered case reaches: {missing}"
    full = tier_selection()
    assert {f: sel[f][0] for f in TIER_REQUIRED} == {f: full[f][0] for f in TIER_REQUIRED}, "not the smallest reduction length"


def test_operand_range_bound_rejects_broken_splits():
    """The inputs and the tolerance of the tiered GPU tests can see what they are for, independently of the kernels: the
    documented fp16 x 2 arithmetic emulated on a plain GEMM (test_gpu_operand_range.emulate_gemm) with tiered operands, at the
    smallest and the largest reduction length the tiered cases use.  The faithful emulation stays within the per-element bound
    c_path U A + F of test_gpu_conv_plans.py; each broken one leaves it on at least one element: fp16 subnormals flushed to zero,
    the low piece dropped below 2^-17 of amax, and s one binade too small for a Winograd-style operand (bounded by
    2^shift amax; one element planted at that bound with amax at the top of its binade: the only place an off-by-one shift
    shows, as an fp16 overflow)."""
    from test_gpu_operand_range import TIER_REQUIRED, emulate_gemm, gemm_bound, tier_selection, tiered_gemm_operands
    sel = tier_selection()
    lengths = [sel[f][0] for f in TIER_REQUIRED]
    for K in (min(lengths), max(lengths)):
        A, B = tiered_gemm_operands(112, K, 112, 20261018)
        ref, tol = A.double() @ B.double(), gemm_bound(A, B)

        def worst(got):
            r = (got.double() - ref).abs() / tol
            return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max().item()

        assert worst(emulate_gemm(A, B)) <= 1.0, f"K = {K}: the faithful emulation leaves the bound"
        for variant in ("flush", "drop_l"):
            assert worst(emulate_gemm(A, B, variant)) > 1.0, f"K = {K}: the bound does not see '{variant}'"
        # the Winograd-style operand: A is bounded by 4 amax(source), the source's amax at the top of its binade and one element
        # of A (tier 0) at the bound, where a 2 x 2 tile of +-amax in the transform's sign pattern puts it
        src_amax = (2.0 - 2.0 ** -12) * 2.0 ** torch.tensor(A.abs().max().item()).log2().ceil().item()
        A[0, 0] = 4.0 * src_amax
        ref, tol = A.double() @ B.double(), gemm_bound(A, B)
        assert worst(emulate_gemm(A, B, a_shift=2, a_amax=src_amax)) <= 1.0, f"K = {K}: shift 2 leaves the bound"
        assert worst(emulate_gemm(A, B, a_shift=1, a_amax=src_amax)) > 1.0, f"K = {K}: the bound does not see a shift of 1 for 2"


def _environment_names_read(path):
    """Names of the environment variables the source file at `path` reads: the first argument of every `os.environ.get` /
    `.setdefault` / `.pop` / `os.getenv` call and every `os.environ[...]` subscript (`os` under any alias)."""
    import ast
    tree = ast.parse(open(path).read(), path)

    def is_environ(node):
        return isinstance(node, ast.Attribute) and node.attr == "environ" and isinstance(node.value, ast.Name)

    names = set()
    for node in ast.walk(tree):
        key = None
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute):
            if (is_environ(node.func.value) and node.func.attr in ("get", "setdefault", "pop")) or \
                    (node.func.attr == "getenv" and isinstance(node.func.value, ast.Name)):
                key = node.args[0]
        elif isinstance(node, ast.Subscript) and is_environ(node.value):
            key = node.slice
        if key is not None:
            assert isinstance(key, ast.Constant) and isinstance(key.value, str), \
                f"{path}:{node.lineno}: an environment variable whose name is not a string literal"
            names.add(key.value)
    return names


def test_the_package_reads_only_the_listed_environment_variables():
    """Every switch the Python package reads from the environment, by name.  A/B switches whose question is settled are
    retired, not kept; a new one has to be added here on purpose."""
    import glob
    listed = {
        # the launcher's (torchrun) and the runtime's
        "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
        "HIP_FORCE_DEV_KERNARG", "GPU_MAX_HW_QUEUES", "HSA_ENABLE_IPC_MODE_LEGACY",
        # the build and the library that is loaded
        "HIPCC", "VCG_LIBVCG",
        # streams (bench.py and tools/*.sh drive them)
        "VCG_WGRAD_OVERLAP", "VCG_DIR_STREAMS",
        # data parallelism
        "VCG_BUCKET_MB", "VCG_DP_FROM_BACKWARD", "VCG_DP_LAUNCH_STREAM", "VCG_NCCL_PRIORITY",
        # input pipeline
        "VCG_HYPERSIM_ALIGNED",
    }
    sources = sorted(glob.glob(os.path.join(ROOT, "vae-cyclegan-implementation_amd", "*.py")))
    assert sources
    read = set()
    for path in sources:
        read |= _environment_names_read(path)
    assert read == listed, f"read but not listed: {sorted(read - listed)}; listed but not read: {sorted(listed - read)}"
