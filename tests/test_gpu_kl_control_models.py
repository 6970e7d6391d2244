"""GPU: the KL controls in the five variational models — free-bits floor (kl_free_bits), annealed weight (kl_anneal_steps,
kl_cycles, kl_ramp) — through configure_loss, training_step, validation_step, a checkpoint round trip and a one-rank process group.

Sizes: batch 2 at 32 x 32 for vae, cyclevae and doublevae (a 2 x 2 latent map, 8 rows); vaegan and cyclevaegan run at 256 x 256,
batch 1, the only size their discriminators' full-map layer accepts (256 rows).  latent_dim 8, and 6 (pad lanes: pitch 8) for
vae and cyclevae.  Weights are the constructors' own draws under a fixed torch seed; a twin is a second instance loaded with the
first one's state_dict before either is configured.  eps comes from the on-device stream, reseeded before every step that is
compared.  lambda_kl is 1 here, so the KL term moves the parameters visibly.

The floor of the free-bits step is the median of the step's own channel KLs: a third instance (the probe) runs one no-grad
validation_step on the batch under the same eps seed with a hook on its KL module, and the channel KLs of every (mu, logvar)
pair it saw are pooled."""
import copy
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LK = 1.0
EPS_SEED = 4321
CASES = [("vae", 8), ("vae", 6), ("cyclevae", 8), ("cyclevae", 6), ("doublevae", 8), ("vaegan", 8), ("cyclevaegan", 8)]


def build(pkg, arch, latent):
    N = pkg.Networks
    return {"vae": lambda: N.VariationalAutoencoder(latent_dim=latent), "vaegan": lambda: N.VAEGAN(latent_dim=latent),
            "cyclevae": lambda: N.CycleVAE(latent_dim=latent, paired=False),
            "cyclevaegan": lambda: N.CycleVAEGAN(latent_dim=latent, paired=False),
            "doublevae": lambda: N.DoubleVariationalAutoencoder(latent_dim=latent)}[arch]()


def instances(pkg, arch, latent, count):
    torch.manual_seed(20261021)
    first = build(pkg, arch, latent)
    sd = {k: v.clone() for k, v in first.state_dict().items()}
    out = [first]
    for _ in range(count - 1):
        m = build(pkg, arch, latent)
        m.load_state_dict(sd)
        out.append(m)
    return out


def ready(model, device, **loss_kw):
    model = model.to(device).train()
    model.configure_optimizers(lr=2e-4)
    model.configure_loss(lambda_kl=LK, **loss_kw)
    return model


def batch_of(pkg, arch, device, index=0):
    n, s = (1, 256) if arch in ("vaegan", "cyclevaegan") else (2, 32)
    x = pkg.ops.rand_uniform((n, 3, s, s), device, seed=77, offset=index << 22)
    y = pkg.ops.rand_uniform((n, 3, s, s), device, seed=77, offset=(index << 22) + (1 << 21))
    return {"x": x, "y": x if arch == "vae" else y}


def gen_optimizer(model):
    return getattr(model, "optimizer_G", None) or model.optimizer


def step(pkg, model, batch, seed=EPS_SEED):
    pkg.ops.manual_seed(seed)
    m = model.training_step(dict(batch))
    torch.cuda.synchronize()
    return m


def kl_module(pkg, model):
    (mod,) = [m for m in model.modules() if isinstance(m, pkg.Losses.KLDivergenceLoss)]
    return mod


def probe_channel_kls(pkg, probe, batch):
    """-> (the pooled channel KLs of the step, sum over the pairs of mean 0.5 (1 + |l| + mu^2 + exp l) for the forward bound)"""
    seen = []
    handle = kl_module(pkg, probe).register_forward_hook(lambda mod, inp, out: seen.append(inp))
    pkg.ops.manual_seed(EPS_SEED)
    with torch.no_grad():
        probe.validation_step(dict(batch))
    handle.remove()
    kls, absum = [], 0.0
    for mu, lv in seen:
        kls.append(pkg.ops.kl_free_bits(mu, lv, 0.0, channel_kl=True)[3].double().cpu())
        m64, l64 = (mu * 1.0).double(), torch.clamp((lv * 1.0).double(), -10, 10)
        absum += (0.5 * (1 + l64.abs() + m64 ** 2 + torch.exp(l64))).mean().item()
    return torch.cat(kls), absum, len(seen)


@pytest.mark.parametrize("arch,latent", CASES)
def test_free_bits_step(arch, latent, pkg, device):
    model, twin, probe = instances(pkg, arch, latent, 3)
    batch = batch_of(pkg, arch, device)
    kls, absum, pairs = probe_channel_kls(pkg, ready(probe, device), batch)
    assert pairs == {"vae": 1, "vaegan": 1, "doublevae": 2, "cyclevae": 4, "cyclevaegan": 4}[arch] and len(kls) == pairs * latent
    del probe
    s = torch.sort(kls).values
    floor = 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]).item()
    assert floor > 0
    twin, model = ready(twin, device), ready(model, device, kl_free_bits=floor)
    mt, mm = step(pkg, twin, batch), step(pkg, model, batch)
    print(f"{arch}/{latent}: floor {floor:.5f} loss_kl {mm['loss_kl']:.6f} (twin {mt['loss_kl']:.6f}) loss_kl_fb {mm['loss_kl_fb']:.6f} "
          f"kl_active {mm['kl_active']:.4f}")
    # loss_kl stays the plain KL: the twin's flat reduction and the per-channel one, each within its forward bound (depth: at most
    # 4 terms per lane and a 10-level tree in the flat kernel, rows per lane + 8 levels in the per-channel one; + 8 per term)
    bound = 2 * U * ((16 + 8) * absum + abs(mt["loss_kl"]))
    assert abs(mm["loss_kl"] - mt["loss_kl"]) <= bound, (mm["loss_kl"], mt["loss_kl"], bound)
    assert mm["loss_kl_fb"] >= mm["loss_kl"]
    assert 0.0 < mm["kl_active"] < 1.0
    assert abs(mm["kl_active"] * pairs * latent - round(mm["kl_active"] * pairs * latent)) < 1e-3       # a count over the channels
    keys = list(mm)
    at = keys.index("loss_kl")
    assert keys[at + 1:at + 3] == ["loss_kl_fb", "kl_active"]
    assert [k for k in keys if k not in ("loss_kl_fb", "kl_active")] == list(mt)
    assert not torch.equal(gen_optimizer(model).flat_param, gen_optimizer(twin).flat_param), "the floor changed no parameter"
    v = model.validation_step(dict(batch))
    vk = [k for k in v if k not in ("Gx", "Fy")]
    assert vk[vk.index("loss_kl") + 1:vk.index("loss_kl") + 3] == ["loss_kl_fb", "kl_active"] and "kl_weight" not in v
    assert v["loss_kl_fb"] >= v["loss_kl"]


@pytest.mark.parametrize("arch", ["vae", "doublevae"])
def test_defaults_are_bit_for_bit_the_model_that_never_heard_of_the_options(arch, pkg, device):
    model, twin = instances(pkg, arch, 8, 2)
    twin = ready(twin, device)
    model = ready(model, device, kl_free_bits=0.0, kl_anneal_steps=0, kl_cycles=1, kl_ramp=1.0)
    for i in range(2):
        batch = batch_of(pkg, arch, device, i)
        mt, mm = step(pkg, twin, batch, EPS_SEED + i), step(pkg, model, batch, EPS_SEED + i)
        assert list(mm) == list(mt) and mm == mt, (mm, mt)
        assert torch.equal(model.optimizer.flat_param, twin.optimizer.flat_param)
        assert torch.equal(model.optimizer.flat_grad, twin.optimizer.flat_grad)
    assert kl_module(pkg, model).plain is None      # the floored kernels never ran


def test_annealed_weight_validation_and_resume(pkg, device):
    at = pkg.optim.kl_weight_at
    model, zero, fresh = instances(pkg, "vae", 8, 3)
    model = ready(model, device, kl_anneal_steps=4)
    zero = zero.to(device).train()
    zero.configure_optimizers(lr=2e-4)
    zero.configure_loss(lambda_kl=0.0)
    batches = [batch_of(pkg, "vae", device, i) for i in range(6)]
    records, saved = [], None
    for t in range(6):
        m = step(pkg, model, batches[t], EPS_SEED + t)
        assert m["kl_weight"] == at(LK, t, 4), (t, m["kl_weight"])
        keys = list(m)
        assert keys[keys.index("loss_kl") + 1] == "kl_weight"
        records.append((m, model.optimizer.flat_param.clone()))
        if t == 0:                                # weight 0: the twin whose lambda_kl is 0, bit for bit
            mz = step(pkg, zero, batches[0], EPS_SEED)
            assert torch.equal(model.optimizer.flat_param, zero.optimizer.flat_param)
            assert m["G_loss"] == mz["G_loss"] and m["loss_kl"] == mz["loss_kl"]
        if t in (0, 2):                           # validation between the steps: the full weight, whatever the schedule says
            pkg.ops.manual_seed(99)
            v = model.validation_step(dict(batches[t]))
            assert "kl_weight" not in v and model.optimizer.step_count == t + 1
            want = v["loss_trans"] + LK * v["loss_kl"]
            assert abs(v["G_loss"] - want) <= 4 * U * want, (v["G_loss"], want)
            assert v["loss_kl"] > 100 * U * want      # the term is visible in the sum
        if t == 2:
            saved = ({k: v.detach().clone() for k, v in model.state_dict().items()}, copy.deepcopy(model.save_optimizer_states()))
    assert [r[0]["kl_weight"] for r in records] == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0]
    # resume into a fresh model: the optimizer's step counter carries the schedule
    fresh.load_state_dict(saved[0])
    fresh = ready(fresh, device, kl_anneal_steps=4)
    fresh.load_optimizer_states(saved[1])
    assert fresh.optimizer.step_count == 3
    for t in range(3, 6):
        m = step(pkg, fresh, batches[t], EPS_SEED + t)
        assert m == records[t][0], (t, m, records[t][0])
        assert torch.equal(fresh.optimizer.flat_param, records[t][1]), f"step {t}: the resumed run left the uninterrupted one"


def test_one_rank_process_group_is_bit_for_bit_the_plain_step(pkg, device, tmp_path):
    import torch.distributed as dist
    kw = dict(kl_free_bits=0.05, kl_anneal_steps=4, kl_cycles=2, kl_ramp=0.5)
    model, plain = instances(pkg, "vae", 6, 2)
    model, plain = ready(model, device, **kw), ready(plain, device, **kw)
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    hook = pkg.ops.GRAD_READY_HOOK[0]
    dist.init_process_group("gloo", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{port}")
    try:
        red = pkg.parallel.attach(model)
        assert red.world == 1
        for t in range(3):
            batch = batch_of(pkg, "vae", device, t)
            mp, mm = step(pkg, plain, batch, EPS_SEED + t), step(pkg, model, batch, EPS_SEED + t)
            assert mm == mp, (t, mm, mp)
            assert {"loss_kl_fb", "kl_active", "kl_weight"} <= set(mm)
            assert torch.equal(model.optimizer.flat_param, plain.optimizer.flat_param)
    finally:
        pkg.ops.GRAD_READY_HOOK[0] = hook
        model.grad_reducer = None
        dist.destroy_process_group()
