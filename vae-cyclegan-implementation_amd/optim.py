"""Fused Adam over one flat fp32 parameter buffer.

Replaces torch.optim.Adam at the reference's call sites (Networks.py:312, 894, 1928-1935:
lr from --lr, betas (0.5, 0.999), eps 1e-8, no weight decay).  All parameters handed to
the optimizer are re-homed as views of a single contiguous buffer; `.grad` of each is a
view of a second buffer that the conv backward kernels accumulate into directly.  One
optimizer step is therefore ONE kernel launch reading/writing 28 B per parameter, and a
data-parallel gradient exchange is an all-reduce over contiguous slices of `flat_grad`.

`max_grad_norm` clips the gradient by its global 2-norm, torch.nn.utils.clip_grad_norm_'s definition, without leaving the
device: one reduction over `flat_grad` (ops.grad_norm) leaves the coefficient in `clip_state`, and the Adam launch reads it
there.

`ema_decay` keeps an exponential moving average of the parameters in a buffer of its own (`flat_ema`), updated by one extra launch
per step (csrc/ema.hip): the Adam kernel is not involved.  `swap_ema()` exchanges the average with the parameters for an evaluation.

`state_dict()` / `load_state_dict()` speak torch.optim.Adam's format (per-parameter
`step`, `exp_avg`, `exp_avg_sq`, one param group) so optimizer states move between the
reference and this implementation.
"""
import math

import torch

from . import ops

_ALIGN = 4  # elements; keeps every view 16-byte aligned for float4 access


def ema_decay_at(ema_decay, updates):
    """The decay of the update that follows `updates` completed ones: 0 for the first (it copies the parameters: whatever was
    loaded or broadcast after the optimizer was built is what the average starts from), then the usual warm-up
    min(ema_decay, (1 + k) / (10 + k)), which climbs from 2/11 to `ema_decay` and stays there."""
    k = int(updates)
    if k <= 0:
        return 0.0
    return min(float(ema_decay), (1.0 + k) / (10.0 + k))


def kl_weight_at(lambda_kl, t, anneal_steps, cycles=1, ramp=1.0):
    """The KL weight of the training step that follows `t` completed generator-optimizer steps.  anneal_steps == 0: lambda_kl,
    always.  Otherwise `cycles` cycles of anneal_steps steps each: within a cycle the weight climbs linearly from 0 over the first
    ramp * anneal_steps steps and stays at lambda_kl for the rest,
        lambda_kl * min(1, ((t mod anneal_steps) / anneal_steps) / ramp)    for t < cycles * anneal_steps,
    and after the last cycle it is lambda_kl.  cycles = 1, ramp = 1: the monotone linear warm-up (Bowman et al. 2016);
    cycles = 4, ramp = 0.5: the cyclical schedule of Fu et al. 2019.  Host arithmetic only."""
    lambda_kl, t, anneal_steps, cycles = float(lambda_kl), int(t), int(anneal_steps), int(cycles)
    if anneal_steps == 0 or t >= cycles * anneal_steps:
        return lambda_kl
    return lambda_kl * min(1.0, ((max(t, 0) % anneal_steps) / anneal_steps) / float(ramp))


class FusedAdam:
    """`max_grad_norm=None`: plain Adam, the launches it always made.  A positive finite float: every step() first measures
    `grad_scale * ||flat_grad||_2` (the gradient Adam sees: the global-batch gradient under data parallelism; the alignment
    padding of the buffer is zero and stays zero) and the Adam launches scale the gradient by min(1, max_grad_norm / (norm + 1e-6)).
    `clip_state` (device, four floats) holds [norm, coefficient, 1.0 if the gradient held a NaN / Inf, 0] of the last step.  A
    step whose gradient holds a NaN or an Inf writes nothing: parameters and moments keep their bits.  The host does not learn of
    it without a synchronisation, so the step counters advance as usual: the price of a skipped step is one step of bias
    correction.  `max_grad_norm` is an attribute of the object only: it is neither in `param_groups` nor in `state_dict()`,
    whose layout is torch.optim.Adam's.

    `ema_decay=None`: no average: no buffer, no launch.  A float in (0, 1): `flat_ema` (the size of `flat_param`, its alignment
    padding zero like the parameters') follows the parameters: after the Adam launches of every step(), ONE launch over the whole
    buffer on the same stream does ema += (1 - d) (param - ema) with d = ema_decay_at(ema_decay, ema_updates).  With clipping
    configured the launch reads `clip_state` too and writes nothing where Adam wrote nothing.  The host cannot see such a skipped
    step, so `ema_updates` advances regardless, as the step counters do: the price is one step of the warm-up schedule.
    The average is not part of `state_dict()` or `param_groups`; `ema_state()` / `load_ema_state()` carry it."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, ema_decay=None):
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not (math.isfinite(ema_decay) and 0.0 < ema_decay < 1.0):
                raise ValueError(f"ema_decay must lie in (0, 1) or be None, got {ema_decay!r}")
        self.ema_decay = ema_decay
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (math.isfinite(max_grad_norm) and max_grad_norm > 0.0):
                raise ValueError(f"max_grad_norm must be a positive finite number or None, got {max_grad_norm!r}")
        self.max_grad_norm = max_grad_norm
        plist = []
        seen = set()
        for p in params:
            if id(p) not in seen:
                seen.add(id(p))
                plist.append(p)
        if not plist:
            raise ValueError("optimizer got an empty parameter list")
        dev = plist[0].device
        if dev.type != "cuda":
            raise RuntimeError("FusedAdam needs parameters on the GPU (call model.to('cuda') before configure_optimizers)")
        for p in plist:
            if p.device != dev or p.dtype != torch.float32:
                raise RuntimeError("FusedAdam: all parameters must be float32 on one device")
        self.params = plist
        self.offsets = []
        off = 0
        for p in plist:
            self.offsets.append(off)
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.total = off
        self.flat_param = torch.empty(off, dtype=torch.float32, device=dev)
        self.flat_grad = torch.empty(off, dtype=torch.float32, device=dev)
        self.exp_avg = torch.empty(off, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.empty(off, dtype=torch.float32, device=dev)
        for buf in (self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq):
            ops.fill_(buf, 0.0)
        with torch.no_grad():
            for p, o in zip(plist, self.offsets):
                view = self.flat_param[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)          # one-time re-homing of the initial values
                p.data = view
                p.grad = self.flat_grad[o:o + p.numel()].view(p.shape)
        self.step_count = 0                     # steps taken by the parameters' common counter (max over `steps`)
        self.steps = [0] * len(plist)           # torch.optim.Adam keeps one counter per parameter; so do we
        self.grad_scale = 1.0
        self._epoch = [0]                       # bumped by step(); ConvSpec.packed() keys its cache on it
        for p in plist:
            p._vcg_epoch = self._epoch
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                             foreach=None, capturable=False, differentiable=False, fused=None,
                             decoupled_weight_decay=False)
        self.param_groups = [dict(self.defaults, params=plist)]
        self.clip_state = None
        if max_grad_norm is not None:
            self.clip_state = torch.empty(4, dtype=torch.float32, device=dev)
            ops.fill_(self.clip_state, 0.0)
            self._clip_ws = ops.grad_norm_workspace(off, dev)
        self.flat_ema = None
        if ema_decay is not None:
            self.flat_ema = torch.empty(off, dtype=torch.float32, device=dev)
            ops.fill_(self.flat_ema, 0.0)
            self.ema_updates = 0
            self.ema_swapped = False              # True while flat_param holds the average (swap_ema)
        ops.PARAM_EPOCH[0] += 1

    # -- torch.optim.Optimizer surface -------------------------------------------------
    def zero_grad(self, set_to_none=False):
        """Gradients are accumulation targets of the backward kernels, so they are zeroed, never dropped."""
        if getattr(self, "_exchange_pending", False):
            raise RuntimeError("zero_grad() while this optimizer's gradient exchange is in flight (parallel.GradReducer): "
                               "finish() the exchange and step() first")
        for p, o in zip(self.params, self.offsets):
            g = p.grad
            if g is None or g.data_ptr() != self.flat_grad.data_ptr() + 4 * o:
                p.grad = self.flat_grad[o:o + p.numel()].view(p.shape)
        ops.fill_(self.flat_grad, 0.0)

    def step(self, grad_scale=None, repack=True):
        """`grad_scale` multiplies the gradient inside the fused launch (1/world after a summing
        all-reduce; parallel.GradReducer sets `self.grad_scale`).  `repack=False` leaves the side-stream repack of
        the conv weights to the caller (ops.repack_async), e.g. until no collective is in flight any more."""
        if self.flat_ema is not None and self.ema_swapped:
            raise RuntimeError("step() while the averaged weights are swapped in (swap_ema / ema_scope): swap them out first")
        g = self.param_groups[0]
        scale = self.grad_scale if grad_scale is None else grad_scale
        self.steps = [t + 1 for t in self.steps]
        self.step_count = max(self.steps)
        if self.clip_state is not None:
            ops.grad_norm(self.flat_grad, scale, self.max_grad_norm, self.clip_state, self._clip_ws)
        # one launch per run of consecutive parameters that share a step counter: ONE launch unless a loaded state
        # carried different counters (a reference run that re-created its optimizer for part of the model)
        i = 0
        while i < len(self.params):
            j = i
            while j + 1 < len(self.params) and self.steps[j + 1] == self.steps[i]:
                j += 1
            lo = self.offsets[i]
            hi = self.offsets[j + 1] if j + 1 < len(self.params) else self.total
            if self.clip_state is not None:
                ops.adam_step_flat_clipped(self.flat_param[lo:hi], self.flat_grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                                           self.steps[i], g["lr"], g["betas"][0], g["betas"][1], g["eps"], scale, self.clip_state)
            else:
                ops.adam_step_flat(self.flat_param[lo:hi], self.flat_grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                                   self.steps[i], g["lr"], g["betas"][0], g["betas"][1], g["eps"], scale)
            i = j + 1
        if self.flat_ema is not None:
            ops.ema_update(self.flat_ema, self.flat_param, 1.0 - ema_decay_at(self.ema_decay, self.ema_updates), self.clip_state)
            self.ema_updates += 1
        self._epoch[0] += 1
        if repack:
            ops.repack_async(self.params)

    # -- averaged weights ---------------------------------------------------------------
    def _require_ema(self, what, swapped=False):
        if self.flat_ema is None:
            raise RuntimeError(f"{what}: this optimizer keeps no average (ema_decay=None)")
        if self.ema_swapped and not swapped:
            raise RuntimeError(f"{what} while the averaged weights are swapped in: swap them out first")

    def _seed_ema(self):
        """An average that no update has reached yet IS the parameters (the first update would copy them anyway)."""
        if self.ema_updates == 0:
            ops.ema_update(self.flat_ema, self.flat_param, 1.0)

    def ema_state(self):
        """{"decay", "updates", "tensors": one clone per parameter, shaped like it}."""
        self._require_ema("ema_state()")
        self._seed_ema()
        return {"decay": self.ema_decay, "updates": self.ema_updates,
                "tensors": [self.flat_ema[o:o + p.numel()].view(p.shape).clone() for p, o in zip(self.params, self.offsets)]}

    def load_ema_state(self, state):
        """What ema_state() returned (tensors on any device).  The decay stays the configured one."""
        self._require_ema("load_ema_state()")
        tensors = list(state["tensors"])
        if len(tensors) != len(self.params):
            raise ValueError(f"averaged weights for {len(tensors)} parameter(s), this optimizer holds {len(self.params)}: "
                             "they were saved for another parameter list")
        for i, (t, p) in enumerate(zip(tensors, self.params)):
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"averaged weight {i} has shape {tuple(t.shape)}, expected {tuple(p.shape)}")
        updates = int(state["updates"])
        if updates < 0:
            raise ValueError(f"averaged weights with a negative update count {updates}")
        with torch.no_grad():
            for t, p, o in zip(tensors, self.params, self.offsets):
                self.flat_ema[o:o + p.numel()].view(p.shape).copy_(t)
        self.ema_updates = updates

    def swap_ema(self):
        """Exchange parameters and average in place (one launch); every weight pack is rebuilt at its next use.  Twice is the
        identity, bit for bit."""
        self._require_ema("swap_ema()", swapped=True)
        if not self.ema_swapped:
            self._seed_ema()
        # What orders the swap: the packs of the last step are written on the weight-gradient side stream (ops.repack_async)
        # and, in a two-direction forward, on the second direction's stream; both READ the parameters.  join_side_streams
        # makes the current stream wait for everything issued on either, so the exchange starts after their last read.  Readers
        # that come later are ordered the usual way: a pack is keyed on the epochs bumped below, is rebuilt on the stream
        # that first needs it, and a forked stream waits for the current one when it forks (ops.DirectionFork).
        ops.join_side_streams()
        ops.swap_(self.flat_param, self.flat_ema)
        self.ema_swapped = not self.ema_swapped
        self._epoch[0] += 1
        ops.PARAM_EPOCH[0] += 1

    def state_dict(self):
        state = {}
        if self.step_count > 0:
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                if self.steps[i] == 0:
                    continue                      # torch creates a parameter's state at its first step
                state[i] = {
                    "step": torch.tensor(float(self.steps[i])),
                    "exp_avg": self.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                    "exp_avg_sq": self.exp_avg_sq[o:o + p.numel()].view(p.shape).clone(),
                }
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self.params)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """torch.optim.Adam's state_dict (ours or the reference's).  The parameter list must be the one the state was
        saved for: a reference checkpoint written after `configure_optimizers(decoder_only=True)` (Networks.py:307-313)
        holds the decoder's tensors only and loads into an optimizer configured the same way.  Per-parameter step
        counters are kept as they are (they may differ, and a parameter without state starts at step 0)."""
        groups = sd["param_groups"]
        n_saved = sum(len(g["params"]) for g in groups)
        if n_saved != len(self.params):
            raise ValueError(f"optimizer state holds {n_saved} parameter(s), this optimizer {len(self.params)}: the state was "
                             "saved for another parameter list (e.g. a reference Autoencoder run with "
                             "configure_optimizers(decoder_only=True) — configure this model the same way before loading)")
        if len(groups) != 1:
            hyper = [(g.get("lr"), tuple(g.get("betas", ())), g.get("eps"), g.get("weight_decay", 0)) for g in groups]
            if len(set(hyper)) != 1:
                raise ValueError("FusedAdam runs one hyper-parameter set over its flat buffer; the loaded state has "
                                 f"{len(groups)} param groups with different lr / betas / eps")
        if groups[0].get("weight_decay", 0) or groups[0].get("amsgrad", False) or groups[0].get("maximize", False):
            raise ValueError("FusedAdam implements plain Adam (no weight decay / amsgrad / maximize), as the reference uses it")
        for k in ("lr", "betas", "eps"):
            if k in groups[0]:
                self.param_groups[0][k] = tuple(groups[0][k]) if k == "betas" else groups[0][k]
        order = [i for g in groups for i in g["params"]]           # saved index of our i-th parameter
        steps = [0] * len(self.params)
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                st = sd["state"].get(order[i], sd["state"].get(str(order[i])))
                if st is None:
                    ops.fill_(self.exp_avg[o:o + p.numel()], 0.0)
                    ops.fill_(self.exp_avg_sq[o:o + p.numel()], 0.0)
                    continue
                if tuple(st["exp_avg"].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state of parameter {i} has shape {tuple(st['exp_avg'].shape)}, expected {tuple(p.shape)}")
                self.exp_avg[o:o + p.numel()].view(p.shape).copy_(st["exp_avg"])
                self.exp_avg_sq[o:o + p.numel()].view(p.shape).copy_(st["exp_avg_sq"])
                t = float(st["step"])
                if abs(t - round(t)) > 1e-3 or t < 0:
                    raise ValueError(f"optimizer state of parameter {i} has a non-integral step counter {t!r}")
                steps[i] = int(round(t))
        self.steps = steps
        self.step_count = max(steps) if steps else 0
