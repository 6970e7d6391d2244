"""Host-side operators: torch.autograd.Function wrappers over the libvcg C ABI.

Tensors keep the reference's LOGICAL shape (N, C, H, W) but live in HBM as NHWC with a
channel pitch that is a multiple of 4 (`nhwc_view`), so every module boundary of
Networks.py is a zero-copy hand-off.  Which tensors are read in place is `can_alias`'s decision; `logical_of` is how a buffer
is declared to be the package's own (pad lanes zero) — read its contract before calling it on a buffer of yours.  torch is used for device memory, streams and the
autograd graph only; every arithmetic op below is a HIP kernel.  There is no fallback:
CPU tensors raise.
"""
import ctypes
import os
import weakref
import math
from typing import NamedTuple

import torch

from . import _native

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
_ACT = {"Identity": ACT_NONE, "ReLU": ACT_RELU, "LeakyReLU": ACT_LEAKY, "Tanh": ACT_TANH, "Sigmoid": ACT_SIGMOID, None: ACT_NONE}

IN_EPS = 1e-5  # nn.InstanceNorm2d default (Networks.py:61)

# bumped whenever parameters change outside torch's version counters (fused Adam step)
PARAM_EPOCH = [0]


def pitch(c):
    return (c + 3) // 4 * 4


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: expected a tensor on the MI355X (cuda) device, got {t.device}; "
                           "this package has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected float32, got {t.dtype}")


# ------------------------------------------------------------------ live kernel timing (bench.py)
# When PROFILE is a list, every launch group below is bracketed by HIP events on the launch
# stream and appended as (family, algorithmic_flops, start_event, end_event).
PROFILE = None


class _timed:
    def __init__(self, family, flops=0.0, tag=""):
        self.family, self.flops, self.tag = family, flops, tag

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.append((self.family, self.flops, self.e0, self.e1, self.tag))


# ------------------------------------------------------------------ workspace
_WS = {}


def _device_index(device):
    return device.index if device.index is not None else torch.cuda.current_device()


def workspace(nbytes, device):
    """One stream-ordered scratch buffer per (device, stream), grown on demand."""
    key = (_device_index(device), torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        n = max(int(nbytes * 1.25) // 4 + 64, 1 << 20)
        buf = torch.empty(n, dtype=torch.float32, device=device)
        _WS[key] = buf
    return buf


# ------------------------------------------------------------------ weight-gradient side stream
# Inside `with wgrad_overlap():` a conv block's weight gradient is issued on a second HIP stream while its data gradient
# (and everything upstream of it) continues on the caller's stream: the two are independent, and one's HBM-bound
# transforms / reduces and launch tails fall under the other's MFMA phases.  Weight gradients only ever accumulate
# into the optimizer's flat buffer, so the one join is at the end of the block (before anything reads `.grad`).
_SIDE = {}
_OVERLAP = [False]
OVERLAP_ENABLED = os.environ.get("VCG_WGRAD_OVERLAP", "1") != "0"     # what `backward_overlapped` does; off = one stream


def _stream_of(table, device):
    """The auxiliary stream `table` (_SIDE, _DIR, _LAUNCH) holds for `device`, created at first use."""
    idx = _device_index(device)
    st = table.get(idx)
    if st is None:
        st = table[idx] = torch.cuda.Stream(device=device)
    return st


def _side_stream(device):
    return _stream_of(_SIDE, device)


def join_side_streams():
    for st in _SIDE.values():
        torch.cuda.current_stream(st.device).wait_stream(st)
    for st in _DIR.values():
        torch.cuda.current_stream(st.device).wait_stream(st)


# ------------------------------------------------------------------ the two translation directions of a cycle model on two streams
# x -> G(x) -> F(G(x)) -> DY and y -> F(y) -> G(F(y)) -> DX share no activation: `DirectionFork` runs the second chain on a stream
# of its own (forward of both directions + discriminators at batch 8: 10.35 -> 8.74 ms, tools/fwd_overlap_probe.py).  Autograd
# runs every backward node on the stream its forward ran on and orders the edges between them, so the two data-gradient chains
# overlap as well; weight gradients of BOTH chains go to the one weight-gradient stream (they accumulate into the same buffers:
# G and F are used by both chains), which is why this needs `wgrad_overlap` — `two_directions()` is false without it — and the
# one accumulation that stays on a chain's stream (bias gradients out of vcg_in_bwd_bias) is atomic.  What the second chain reads
# that is produced after the fork and is not an autograd edge must be ordered by hand: weight packs and the fused mu / logvar
# weights carry events (`ConvSpec.packed`, `FusedConvPair.tensors`), the images' magnitudes are measured before the fork
# (`premeasure`).  VCG_DIR_STREAMS=0: one chain after the other, as in rounds 1-3.
DIRECTION_STREAMS = os.environ.get("VCG_DIR_STREAMS", "1") != "0"
_DIR = {}


def two_directions():
    return DIRECTION_STREAMS and OVERLAP_ENABLED


class DirectionFork:
    def __init__(self, device):
        self.second_stream = _stream_of(_DIR, device)
        self.main = torch.cuda.current_stream(device)
        self.second_stream.wait_stream(self.main)   # everything issued so far (inputs, zeroed gradients, the optimizer's writes)

    def second(self):
        """Context: issue on the second chain's stream (no wait: the chains are independent after the fork)."""
        return torch.cuda.stream(self.second_stream)

    def join(self):
        self.main.wait_stream(self.second_stream)


_LAUNCH = {}


def launch_stream(device):
    """The stream parallel.GradReducer issues its collectives under (it waits for a bucket's producer streams; nothing but RCCL
    waits for it)."""
    return _stream_of(_LAUNCH, device)


def create_streams(device):
    """Create the step's auxiliary streams now instead of at first use.  DIAGNOSTIC ONLY (bench.py VCG_PRECREATE=1): creating
    them before `init_process_group` looked like the way to give each a hardware queue of its own ahead of the dozens of
    streams a process group brings — and measured 42.8 ms per step against 34.3 with lazy creation (one-rank RCCL group, three
    alternations, profiles/r04_dp_one_rank.txt).  The runtime's stream-to-queue assignment is not something this package can
    steer; what it does control is GPU_MAX_HW_QUEUES (package __init__)."""
    _side_stream(device)
    DirectionFork(device)
    launch_stream(device)


def premeasure(t):
    """Publish the largest magnitude of `t` now, on the current stream, unless a valid handle is already on it: a tensor that
    two streams will read must not be measured by one of them after they have forked."""
    if t.is_cuda and not _amax_of(t):
        _amax_tag(t, _measured_amax(t, logical=True))


class wgrad_overlap:
    def __enter__(self):
        self.prev = _OVERLAP[0]
        _OVERLAP[0] = True
        return self

    def __exit__(self, *exc):
        _OVERLAP[0] = self.prev
        join_side_streams()
        return False


def backward_overlapped(loss, overlap=True, **kw):
    """loss.backward(**kw) with the weight gradients on the side stream (joined before returning).
    `overlap=False`: one stream."""
    if OVERLAP_ENABLED and overlap:
        with wgrad_overlap():
            loss.backward(**kw)
    else:
        loss.backward(**kw)


# ------------------------------------------------------------------ layout
def nhwc_strides(n, c, h, w):
    p = pitch(c)
    return (h * w * p, 1, w * p, p)


def is_nhwc_view(t):
    """Do the STRIDES of t say NHWC at the channel pitch?  Strides alone do not make t the package's storage: `can_alias` decides."""
    n, c, h, w = t.shape
    return t.stride() == nhwc_strides(n, c, h, w)


def _own_pad_lanes(storage, c=None):
    """The mark on a storage whose pad lanes (channels c .. pitch(c) - 1 of every pixel) are the package's own: written as zeros
    by the kernel that filled it, or never read as data.  `c` given: leave the mark (`logical_of`); -> the marked channel count.
    It sits on the storage, not on a tensor object, so a detach(), a batch slice or a saved tensor of the view keeps it, and
    whatever torch allocates itself (a sum of two gradients, a clone, a slice of somebody's RGBA image) never has it."""
    if c is not None:
        storage._vcg_pad_c = c
    return getattr(storage, "_vcg_pad_c", None)


def can_alias(t):
    """May the kernels read logical (N, C, H, W) `t` in place as the physical (N, H, W, pitch(C)) buffer `phys_of` describes?  The
    one decision behind `as_phys`, `to_nhwc` and `to_nchw_contiguous`; pure host logic, any device.  All of:
      * the strides are the NHWC strides at the channel pitch (size-1 dimensions included: torch may give those other strides,
        and such a tensor takes the copy);
      * the alias starts on a 16-byte boundary (the kernels load float4) and its N * H * W * pitch floats end inside the storage
        (a channel slice x4[:, 1:4] of an RGBA image has the right strides and would end one float past it);
      * there are no pad lanes (pitch(C) == C), or they are known to be the package's own zeros: the storage carries the mark
        `logical_of` leaves, for this C.  x4[:, :3] has the strides of a pitch-4 RGB image with alpha in the pad lane, which
        the reductions (L1, InstanceNorm statistics, operand maxima) would take for data: it is copied, never aliased."""
    if t.dim() != 4:
        return False
    n, c, h, w = t.shape                      # (written out flat: this runs for every operand of every Function of a step)
    p = (c + 3) // 4 * 4
    hwp = h * w * p
    if t.stride() != (hwp, 1, w * p, p):
        return False
    off = t.storage_offset()
    if off % 4 or t.data_ptr() % 16:
        return False
    st = t.untyped_storage()
    if (off + n * hwp) * t.element_size() > st.nbytes():
        return False
    return p == c or getattr(st, "_vcg_pad_c", None) == c


def phys_of(t):
    """(N,H,W,P) contiguous alias of a logical (N,C,H,W) nhwc view (one `can_alias` admits)."""
    n, c, h, w = t.shape
    p = pitch(c)
    return t.as_strided((n, h, w, p), (h * w * p, w * p, p, 1), t.storage_offset())


def logical_of(phys, c):
    """The logical (N, c, H, W) view of the physical (N, H, W, P) buffer `phys`.

    CONTRACT: calling it DECLARES the buffer to be in the package's layout.  Where P != c the caller vouches that the pad lanes
    c .. P - 1 of every pixel are zeros by the time a kernel reads the view, or that only kernels that never look at them will
    (the running statistics of translate.py, which `vcg_sample_accumulate` writes whole; the fake tensors of custom_ops).  The
    storage is marked with c (`_own_pad_lanes`), and `can_alias` then hands the buffer to the kernels in place — the reductions
    (L1, InstanceNorm statistics, operand maxima) run over the whole pitch and take whatever the pad lanes hold for data.
    One mark per storage: viewing one storage at two different c sends the earlier view down the (correct, slower) copy path.
    The mark is a Python attribute of the storage object, which torch keeps alive with the storage; a storage that arrives
    without it (pickled, deep-copied) is simply copied."""
    n, h, w, p = phys.shape
    if p != c:
        _own_pad_lanes(phys.untyped_storage(), c)
    return phys.as_strided((n, c, h, w), (h * w * p, 1, w * p, p), phys.storage_offset())


def _to_phys_copy(t):
    """NCHW (any strides) -> fresh NHWC physical tensor, pad channels zeroed."""
    _require_gpu(t, "to_nhwc")
    n, c, h, w = t.shape
    src = t.contiguous()
    p = pitch(c)
    dst = torch.empty((n, h, w, p), dtype=torch.float32, device=t.device)
    _native.check(_native.lib().vcg_nchw_to_nhwc(_ptr(src), _ptr(dst), n, c, h, w, p, _stream()), "vcg_nchw_to_nhwc")
    return dst


def as_phys(t):
    """Physical NHWC tensor for a logical NCHW tensor: alias if already laid out, else convert."""
    if t.dim() != 4:
        raise RuntimeError(f"expected a 4-D (N,C,H,W) tensor, got shape {tuple(t.shape)}")
    _require_gpu(t, "as_phys")
    if can_alias(t):
        return phys_of(t)
    return _to_phys_copy(t)


def to_nchw_contiguous(t):
    """Logical (N,C,H,W) nhwc view -> plain contiguous NCHW copy."""
    _require_gpu(t, "to_nchw")
    if not can_alias(t):
        return t.contiguous()
    n, c, h, w = t.shape
    ph = phys_of(t)
    dst = torch.empty((n, c, h, w), dtype=torch.float32, device=t.device)
    _native.check(_native.lib().vcg_nhwc_to_nchw(_ptr(ph), _ptr(dst), n, c, h, w, pitch(c), _stream()), "vcg_nhwc_to_nchw")
    return dst


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return logical_of(_to_phys_copy(x), x.shape[1])

    @staticmethod
    def backward(ctx, g):
        return to_nchw_contiguous(g)


def to_nhwc(x):
    """x.to(channels-last) with pitch-4 images; differentiable; no-op when already laid out."""
    if x.is_cuda and can_alias(x):
        return x
    _require_gpu(x, "to_nhwc")
    return _ToNHWC.apply(x)


# ------------------------------------------------------------------ conv block
def _param_key(p):
    """What a copy derived from parameter `p` (a weight pack, the fused mu / logvar weights) is valid for: parameters owned by a
    FusedAdam carry that optimizer's step counter (`_vcg_epoch`), so a step of one optimizer does not invalidate what was
    derived from another's parameters."""
    ep = getattr(p, "_vcg_epoch", None)
    return (ep[0] if ep is not None else PARAM_EPOCH[0], id(ep), p._version, p.data_ptr())


class _WrittenOn:
    """Where and when a buffer that several streams read was last written: the writer `mark`s, a reader on another stream
    waits for that event (`order_reader`); a reader on the writer's stream is ordered already."""

    def __init__(self):
        self.stream = self.event = None

    def mark(self, device):
        self.stream = torch.cuda.current_stream(device)
        self.event = torch.cuda.Event()
        self.event.record(self.stream)

    def order_reader(self, device):
        if self.event is not None:
            cur = torch.cuda.current_stream(device)
            if cur != self.stream:
                cur.wait_event(self.event)


class ConvSpec:
    """Static description of one conv (+ fused activation / InstanceNorm / shuffle) block."""

    def __init__(self, cin, cout, k, stride=1, pad=1, reflect=True, ups=1, epi_act=ACT_NONE, norm=False,
                 post_act=ACT_NONE, shuffle=False):
        self.cin, self.cout, self.k = cin, cout, k          # logical channels of the torch conv
        self.stride, self.pad, self.reflect, self.ups = stride, pad, reflect, ups
        self.epi_act, self.norm, self.post_act, self.shuffle = epi_act, norm, post_act, shuffle
        if ACT_SIGMOID in (epi_act, post_act) and pitch(cout) != cout:
            # the activation runs over the whole pitch and sigmoid(0) = 0.5: the pad lanes of the output would not be the zeros
            # every consumer counts on (L1 over the physical buffer, operand maxima, InstanceNorm statistics)
            raise RuntimeError(f"ConvSpec: a Sigmoid block needs a multiple of 4 output channels, got {cout}: sigmoid(0) = 0.5 "
                               "would be written into the pad lanes of the output")
        if ups == 2:
            assert cin % 4 == 0
            self.cin_phys_log = cin // 4                   # channels of the un-shuffled input
        else:
            self.cin_phys_log = cin
        self.cin_pitch = pitch(self.cin_phys_log)
        self.cout_pitch = pitch(cout)
        self._packed = None
        self._packed_key = None
        self._pack_written = _WrittenOn()
        self._pack_weight = None
        self._need_wf = False            # some geometry this spec has run at reads the fp32 Wf block of the pack (sticky)
        self._wf_packed = False          # the current pack holds it
        self._geoms_seen = set()

    def desc(self, n, h, w):
        cd = (ctypes.c_int32 * 16)()
        cd[0], cd[1], cd[2] = n, h, w
        cd[3], cd[4] = self.cin_pitch, self.cout_pitch
        cd[5], cd[6], cd[7], cd[8] = self.k, self.k, self.stride, self.pad
        cd[9], cd[10], cd[11] = int(self.reflect), self.ups, self.epi_act
        cd[12], cd[13] = self.cin_phys_log, self.cout
        return cd

    def out_hw(self, h, w):
        hl, wl = h // self.ups, w // self.ups
        return ((hl + 2 * self.pad - self.k) // self.stride + 1, (wl + 2 * self.pad - self.k) // self.stride + 1)

    def packed(self, weight, geom=None):
        """Packed weight buffer (Wf + the transformed copies) for the current parameter values: repacked once per
        optimizer step (`_param_key`).
        `geom` = (n, h, w) of the call that is about to use the pack: the fp32 Wf block is only written for specs some
        geometry of which reads it (include/vcg.h, vcg_conv_reads_wf: the D / R / U layers run from their planes in every
        direction — a third of the pack traffic of a step; against packs that always carry it, same box twice: 36.82 / 36.74 ->
        36.61 / 36.64 ms per step, -0.55 ms of side-stream pack kernels, -1 GB).  No geometry given (tests, `repack_async`):
        what is known so far."""
        if geom is not None and geom not in self._geoms_seen:
            self._geoms_seen.add(geom)
            if not self._need_wf and _native.lib().vcg_conv_reads_wf(self.desc(*geom)):
                self._need_wf = True
        want_wf = self._need_wf or not self._geoms_seen       # never used through a geometry yet: the full pack
        key = _param_key(weight)
        if self._packed is None or self._packed_key != key or self._packed.device != weight.device or (want_wf and not self._wf_packed):
            cd = self.desc(1, max(self.ups * self.k, 2 * self.ups * (self.pad + 1)), max(self.ups * self.k, 2 * self.ups * (self.pad + 1)))
            cd[14] = 0 if want_wf else 1                                   # VCG_CD_PACK_FLAGS
            if self._packed is None or self._packed.device != weight.device:
                nfl = int(_native.lib().vcg_pack_weight_floats(cd))
                if nfl <= 0:
                    raise RuntimeError(f"vcg_pack_weight_floats failed: {_native.lib().vcg_last_error().decode()}")
                self._packed = torch.empty(nfl, dtype=torch.float32, device=weight.device)
            w = weight.detach()
            if not w.is_contiguous():
                w = w.contiguous()
            _native.check(_native.lib().vcg_pack_weight(_ptr(w), _ptr(self._packed), cd, _stream()), "vcg_pack_weight")
            self._wf_packed = want_wf
            self._packed_key = key
            self._pack_written.mark(weight.device)
            self._pack_weight = weakref.ref(weight)
            _PACKS[id(self)] = self
        else:
            self._pack_written.order_reader(weight.device)      # packed ahead of time on the side stream (repack_async)
        return self._packed


_PACKS = weakref.WeakValueDictionary()      # specs that have packed something (dropped with their module)


def repack_async(params):
    """After an optimizer step: repack the conv weights that step changed, on the side stream, so that the next
    forward finds them ready (each consumer waits on its own pack's event) instead of packing layer by layer on its
    critical path."""
    if not OVERLAP_ENABLED or not _PACKS:
        return
    ids = {id(p) for p in params}
    todo = []
    for sp in list(_PACKS.values()):
        w = sp._pack_weight() if sp._pack_weight is not None else None
        if w is not None and id(w) in ids and w.is_cuda:
            todo.append((sp, w))
    if not todo:
        return
    dev = todo[0][1].device
    side = _side_stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))        # after the Adam launch and after every reader of the old packs
    with torch.cuda.stream(side):
        for sp, w in todo:
            sp.packed(w)


# Hand the largest magnitude of an activation / gradient from the kernel that wrote it to the convolution that reads it
# (include/vcg.h, vcg_amax_hint).  False (an A/B run or a test sets the attribute): every convolution measures its operands itself.
# Consulted by `_amax_of`, `_measured_amax` and `_amax_out` below and nowhere else: with handles off they deal in 0, "unknown",
# which `_amax_tag`, every caller and the library already take.
AMAX_HANDLES = True


def _amax_tag(t, handle):
    """Leave `handle` on tensor object `t`, keyed on what it describes: the contents of this storage at this version.  torch bumps
    `_version` on every in-place write through any view of the storage, so `h = block(x); h.mul_(8); block2(h)` finds a version
    mismatch and measures (round 3 kept the bare handle: a stale amax scaled the operand into fp16 overflow — VERDICT r3 weak #8)."""
    if handle:
        try:
            t._vcg_amax = (int(handle), t._version, t.data_ptr())
        except AttributeError:
            pass


def _amax_of(t):
    """The handle left on `t` if it still describes it: same storage, no in-place write since, and young enough for the library
    to honour (an old one is dropped here so that the caller measures ONCE and re-tags, instead of every consumer refusing it)."""
    if not AMAX_HANDLES:
        return 0
    tag = getattr(t, "_vcg_amax", None)
    if not tag:
        return 0
    handle, ver, ptr = tag
    if ver != t._version or ptr != t.data_ptr() or not _native.lib().vcg_amax_valid(handle):
        try:
            del t._vcg_amax
        except AttributeError:
            pass
        return 0
    return handle


def _measured_amax(t, logical=False):
    """Handle of the largest magnitude of a tensor no kernel published one for (an image, a latent, the gradient a loss hands
    down): measured ONCE on the current stream — the forward and the weight gradient that re-reads x, the weight and the data
    gradient of one dy, two convolutions of one input all take the handle instead of a pass each (round 3: 128 -> ~75 k_absmax
    launches per step).  0 (the consumers measure) when handles are off.  `logical`: t is a logical (N, C, H, W) tensor."""
    if not AMAX_HANDLES:
        return 0
    if logical:
        t = as_phys(t)
    return int(_native.lib().vcg_amax_measure(_ptr(t), t.numel(), _stream()))


def _amax_out(cell):
    """The handle a kernel returned through the pointer to `cell` (a c_uint64) — 0 when handles are off."""
    return cell.value if AMAX_HANDLES else 0


# Data parallelism: parallel.GradReducer.note — told about every weight gradient the backward has issued (and on which
# stream), so that a gradient bucket can be exchanged as soon as its last contribution is in flight.
GRAD_READY_HOOK = [None]


# Phase control of the alternating GAN update.  `ctx.needs_input_grad` is fixed at forward
# time, so the G phase (which needs only the discriminators' data gradient) and the D phase
# (which must not spend a data gradient on the generators' images) say so explicitly.
_NO_WGRAD = set()
_NO_DGRAD = set()


class no_wgrad:
    """Within this context the backward skips weight/bias gradients of these parameters."""

    def __init__(self, params):
        self.ids = [id(p) for p in params]

    def __enter__(self):
        _NO_WGRAD.update(self.ids)

    def __exit__(self, *a):
        _NO_WGRAD.difference_update(self.ids)


class no_dgrad:
    """Within this context the backward skips the input gradient of these ConvSpecs."""

    def __init__(self, specs):
        self.ids = [id(s) for s in specs]

    def __enter__(self):
        _NO_DGRAD.update(self.ids)

    def __exit__(self, *a):
        _NO_DGRAD.difference_update(self.ids)


def _grad_buffer(param):
    """param.grad as an accumulation target (allocated zeroed on first use)."""
    if param.grad is None:
        param.grad = torch.zeros_like(param, memory_format=torch.contiguous_format)
    g = param.grad
    if not g.is_contiguous():
        raise RuntimeError("parameter .grad must be contiguous")
    return g


# ------------------------------------------------------------------ the conv block's library calls, each written once
# Mechanism only ("One call site per library call of the conv block"): plain functions over PHYSICAL tensors that
# allocate their outputs, issue one group of library calls on the current stream inside its `_timed` bracket and return the
# results.  Operand magnitudes come in and go out as bare handles (0: unknown, the kernels measure).  What decides about
# tensor tags, deferral, the kept forward state, streams, parameters and hooks is `_ConvBlockFn`; `custom_ops` is the same
# sequence with none of that.  `flops`, `tag` = `conv_cost(...)`: what the bracket of a convolution reports.
def conv_cost(spec, n, h, w):
    """(algorithmic flops, tag) of one direction of `spec` on an (n, h, w) input."""
    ho, wo = spec.out_hw(h, w)
    return (2.0 * n * ho * wo * spec.cout * spec.k * spec.k * spec.cin,
            f"{n}x{h}x{w}x{spec.cin_pitch}->{spec.cout_pitch} k{spec.k} s{spec.stride} u{spec.ups}")


def conv_forward(spec, cd, wf, bias, xp=None, x_amax=0, lazy=None, want_stats=False, saved=None, flops=0.0, tag=""):
    """The convolution (+ bias, + epilogue activation) of `xp`, whose largest magnitude handle `x_amax` names — or, with
    `lazy` = (t_prev, mean, rstd, act, ...), of the producer's raw output normalised in this convolution's own gather — and, if
    `want_stats`, the statistics of the InstanceNorm that follows, out of the conv's own epilogue where its launch plan allows
    (csrc/conv_igemm.hip, vcg_conv_fwd_in).  `saved`: buffer for the forward state the weight gradient reuses, or None.
    -> (t, mean, rstd); the last two None without statistics."""
    lib = _native.lib()
    n, (ho, wo), c, dev = cd[0], spec.out_hw(cd[1], cd[2]), spec.cout_pitch, wf.device
    t = torch.empty((n, ho, wo, c), dtype=torch.float32, device=dev)
    mean = rstd = None
    if want_stats:
        mean = torch.empty((n, c), dtype=torch.float32, device=dev)
        rstd = torch.empty((n, c), dtype=torch.float32, device=dev)
    with _timed("conv_fwd", flops, tag):
        ws = workspace((lib.vcg_conv_fwd_in_workspace if want_stats else lib.vcg_conv_fwd_workspace)(cd), dev)
        if lazy is not None:
            _native.check(lib.vcg_conv_fwd_in_pre(_ptr(lazy[0]), _ptr(lazy[1]), _ptr(lazy[2]), lazy[3], _ptr(wf), _ptr(bias),
                                                  _ptr(t), _ptr(mean), _ptr(rstd), IN_EPS, _ptr(saved), cd, _ptr(ws),
                                                  ws.numel() * 4, _stream()), "vcg_conv_fwd_in_pre")
        else:
            _native.check(lib.vcg_conv_fwd_in_h(_ptr(xp), _ptr(wf), _ptr(bias), _ptr(t), _ptr(mean), _ptr(rstd), IN_EPS,
                                                _ptr(saved), cd, _ptr(ws), ws.numel() * 4, x_amax, _stream()), "vcg_conv_fwd_in")
    return t, mean, rstd


def norm_out(t, cout, shuffle=False):
    """Storage for the InstanceNorm's result on the raw conv output `t` of `cout` logical channels -> (outp, logical channels)."""
    if not shuffle:
        return torch.empty_like(t), cout
    n, ho, wo, c = t.shape
    return torch.empty((n, 2 * ho, 2 * wo, c // 4), dtype=torch.float32, device=t.device), cout // 4


def norm_apply(t, mean, rstd, act, cout, resp=None, shuffle=False, outp=None):
    """act((t - mean) * rstd) (+ residual `resp`), stored pixel-shuffled if `shuffle`, into `outp` (default: fresh storage).
    -> (outp, logical channels, handle of its largest magnitude)."""
    if outp is None:
        outp, cout = norm_out(t, cout, shuffle)
    n, ho, wo, c = t.shape
    amax = ctypes.c_uint64(0)
    with _timed("in_fwd"):
        _native.check(_native.lib().vcg_in_apply_h(_ptr(t), _ptr(mean), _ptr(rstd), _ptr(resp), _ptr(outp), n, ho, wo, c, act,
                                                   int(shuffle), ctypes.byref(amax), _stream()), "vcg_in_apply")
    return outp, cout, _amax_out(amax)


def block_dt(spec, gp, t, mean, rstd, gb=None):
    """The gradient at the convolution's output from the block's output gradient `gp`: through the InstanceNorm (+ both
    activations), through the epilogue activation alone (`t` is then the activation's output), or `gp` itself.  `gb`: a bias
    gradient buffer to accumulate dt's column sums into in the same pass (vcg_in_bwd_bias), or None: not taken here.
    -> (dt, handle of its largest magnitude: 0 for a passed-through gp)."""
    lib = _native.lib()
    if not spec.norm and spec.epi_act == ACT_NONE:
        return gp, 0
    dt = torch.empty_like(t)
    h = ctypes.c_uint64(0)
    if not spec.norm:
        _native.check(lib.vcg_act_bwd_h(_ptr(gp), _ptr(t), _ptr(dt), t.numel(), spec.epi_act, ctypes.byref(h), _stream()), "vcg_act_bwd")
        return dt, _amax_out(h)
    n, ho, wo, c = t.shape
    ws = workspace(lib.vcg_in_workspace(n, ho * wo, c), t.device)
    with _timed("in_bwd"):
        if gb is not None:
            _native.check(lib.vcg_in_bwd_bias(_ptr(gp), _ptr(t), _ptr(mean), _ptr(rstd), _ptr(dt), n, ho, wo, c,
                                              spec.epi_act, spec.post_act, int(spec.shuffle), _ptr(gb), spec.cout,
                                              _ptr(ws), ws.numel() * 4, ctypes.byref(h), _stream()), "vcg_in_bwd_bias")
        else:
            _native.check(lib.vcg_in_bwd_h(_ptr(gp), _ptr(t), _ptr(mean), _ptr(rstd), _ptr(dt), n, ho, wo, c,
                                           spec.epi_act, spec.post_act, int(spec.shuffle), _ptr(ws), ws.numel() * 4,
                                           ctypes.byref(h), _stream()), "vcg_in_bwd")
    return dt, _amax_out(h)


def conv_wgrad(cd, xp, dt, gw, gb, saved=None, x_amax=0, dt_amax=0, flops=0.0, tag=""):
    """Accumulate the weight gradient into `gw` and, unless `gb` is None, the bias gradient (dt's column sums) into `gb`;
    `saved`: the forward state `conv_forward` kept, or None (recomputed)."""
    lib = _native.lib()
    ws = workspace(lib.vcg_conv_wgrad_workspace(cd), dt.device)
    with _timed("conv_wgrad", flops, tag):
        _native.check(lib.vcg_conv_wgrad_saved_h(_ptr(xp), _ptr(dt), _ptr(gw), _ptr(gb), _ptr(saved), cd, _ptr(ws),
                                                 ws.numel() * 4, x_amax, dt_amax, _stream()), "vcg_conv_wgrad")


def conv_dgrad(cd, dt, wf, dt_amax=0, flops=0.0, tag=""):
    """-> the gradient at the convolution's (physical) input."""
    lib = _native.lib()
    dxp = torch.empty((cd[0], cd[1], cd[2], cd[3]), dtype=torch.float32, device=dt.device)
    with _timed("conv_dgrad", flops, tag):
        ws = workspace(lib.vcg_conv_dgrad_workspace(cd), dt.device)
        _native.check(lib.vcg_conv_dgrad_h(_ptr(dt), _ptr(wf), _ptr(dxp), cd, _ptr(ws), ws.numel() * 4, dt_amax,
                                           _stream()), "vcg_conv_dgrad")
    return dxp


# ------------------------------------------------------------------ deferred InstanceNorm (the fused Conv + IN + act hand-off)
# A block whose only consumer is the next block's convolution can hand over its RAW conv output with the statistics instead of the
# normalised tensor: `conv_block(..., defer=True)` returns a tensor whose storage is allocated but NOT written, tagged with
# (t, mean, rstd, post_act); a `conv_block` that receives it normalises inside its own input gather (include/vcg.h,
# vcg_conv_fwd_in_pre) where that exists for its geometry, and otherwise fills the storage first (`materialize`) — so every
# conv_block consumer is correct either way, and nothing else may be handed a deferred tensor (Networks.py defers only between
# the blocks of one Encoder / inside R).  False (an A/B run or a test sets the attribute): never defer.
DEFER_NORM = True


def _lazy_of(x):
    tag = getattr(x, "_vcg_lazy", None)
    if tag is None:
        return None
    t, mean, rstd, act, ver, ptr = tag
    if ver != x._version or ptr != x.data_ptr():
        raise RuntimeError("a deferred-InstanceNorm tensor was written to before its consumer ran")
    return tag


def materialize(x):
    """Fill a deferred tensor's storage with the normalised values (what the producer would have written)."""
    tag = _lazy_of(x)
    if tag is None:
        return x
    t, mean, rstd, act, _, _ = tag
    _, _, amax = norm_apply(t, mean, rstd, act, x.shape[1], outp=phys_of(x))
    del x._vcg_lazy
    _amax_tag(x, amax)
    return x


def consumer_takes_deferred(spec, n, h, w, needs_wgrad=True):
    """Would `conv_block(x, ..., spec)` on an (n, C, h, w) input normalise a deferred x in its gather?  (Asked by the producer's
    caller before deferring: a deferral the consumer cannot use costs nothing but buys nothing.)"""
    if not DEFER_NORM:
        return False
    cache = spec.__dict__.setdefault("_pre_ok", {})        # on the spec itself: an id()-keyed table outlives its specs
    ok = cache.get((n, h, w))
    if ok is None:
        lib = _native.lib()
        cd = spec.desc(n, h, w)
        ok = bool(lib.vcg_conv_pre_ok(cd)), int(lib.vcg_conv_saved_floats(cd)) > 0
        cache[(n, h, w)] = ok
    return ok[0] and (ok[1] or not needs_wgrad)


class _ConvBlockFn(torch.autograd.Function):
    """conv(+bias)(+act) -> [InstanceNorm (+act) (+residual) (+PixelShuffle store)].

    Weight/bias gradients are ACCUMULATED straight into `.grad` (which the fused optimizer
    keeps as views of one flat buffer), so autograd receives None for them.
    """

    @staticmethod
    def forward(ctx, x, weight, bias, residual, spec, wparam, bparam, defer=False):
        if not spec.norm and (residual is not None or spec.shuffle or spec.post_act):
            raise RuntimeError("residual/shuffle/post_act need norm=True")
        if defer and (residual is not None or spec.shuffle):
            raise RuntimeError("a block with a residual or a shuffled store cannot defer its InstanceNorm")
        # (grad mode is off inside Function.forward: needs_input_grad[1] says whether a backward for the weight will come)
        wants_wgrad = wparam is not None and wparam.requires_grad and ctx.needs_input_grad[1]
        lazy = _lazy_of(x)
        if lazy is not None and not consumer_takes_deferred(spec, x.shape[0], x.shape[2], x.shape[3], wants_wgrad):
            materialize(x)
            lazy = None
        xp = as_phys(x)
        n, h, w, pin = xp.shape
        if pin != spec.cin_pitch:
            raise RuntimeError(f"conv block expected {spec.cin_phys_log} input channels (pitch {spec.cin_pitch}), got pitch {pin}")
        cd = spec.desc(n, h, w)
        wf = spec.packed(weight, (n, h, w))
        flops, tag = conv_cost(spec, n, h, w)
        # operand magnitudes (include/vcg.h): the block that wrote x left a handle to its largest magnitude on the tensor; the
        # kernels scale x by it instead of measuring x again (0: unknown, they measure)
        x_amax = 0
        if lazy is None:
            x_amax = _amax_of(x)
            if not x_amax:
                x_amax = _measured_amax(xp)
                _amax_tag(x, x_amax)          # a second convolution of this very tensor object (mu and logvar read one map)
        # forward state the weight gradient reuses (the Winograd-transformed input V: 4x the activation — HBM is 288 GB).
        # Always kept: recomputing it in the weight gradient, as round 1 did, measured 169.0 against 171.0 images/s.
        saved = None
        if wants_wgrad:
            nsv = int(_native.lib().vcg_conv_saved_floats(cd))
            if nsv:
                saved = torch.empty(nsv, dtype=torch.float32, device=x.device)
        t, mean, rstd = conv_forward(spec, cd, wf, bias, xp, x_amax, lazy, spec.norm, saved, flops, tag)
        out_amax = 0
        if not spec.norm:
            outp, cout_log = t, spec.cout
        elif defer:
            outp, cout_log = norm_out(t, spec.cout)      # allocated, not written
        else:
            resp = as_phys(residual) if residual is not None else None
            outp, cout_log, out_amax = norm_apply(t, mean, rstd, spec.post_act, spec.cout, resp, spec.shuffle)
        ctx.spec, ctx.cd, ctx.flops, ctx.tag = spec, cd, flops, tag
        ctx.wparam, ctx.bparam = wparam, bparam
        ctx.has_res = residual is not None
        ctx.saved_state = saved
        # the backward re-reads x (weight gradient): the handle describes x as it is NOW — keep what it is keyed on
        ctx.x_amax, ctx.x_key = x_amax, (xp._version, xp.data_ptr())
        ctx.save_for_backward(xp, t, mean, rstd, wf)
        out = logical_of(outp, cout_log)
        ctx.x_deferred = lazy is not None
        if defer and spec.norm:
            # the storage of `out` stays unwritten: its consumer normalises t in its own gather, or fills it (materialize)
            out._vcg_lazy = (t, mean, rstd, spec.post_act, out._version, out.data_ptr())
        else:
            _amax_tag(out, out_amax)          # for the block that consumes this very tensor object
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _native.lib()
        spec, cd = ctx.spec, ctx.cd
        xp, t, mean, rstd, wf = ctx.saved_tensors
        dev = t.device
        gp = as_phys(g)
        d_res = g if ctx.has_res else None
        wparam, bparam = ctx.wparam, ctx.bparam
        want_w = wparam is not None and wparam.requires_grad and id(wparam) not in _NO_WGRAD
        # A trainable bias under a frozen weight still gets its gradient: from the InstanceNorm backward where that takes it
        # (`gb_here`), else from the weight gradient's own column sums, whose weight part then goes to scratch and is dropped.
        bias_alone = (not want_w and wparam is not None and not wparam.requires_grad and bparam is not None
                      and bparam.requires_grad and id(bparam) not in _NO_WGRAD)
        want_b = (want_w or bias_alone) and bparam is not None and bparam.requires_grad
        run_wgrad = want_w or (bias_alone and not spec.norm)
        if run_wgrad and ctx.x_deferred and ctx.saved_state is None:
            # refused before anything is accumulated: the InstanceNorm backward below already adds into the bias gradient
            raise RuntimeError("the weight gradient of a layer that took a deferred-InstanceNorm input needs the forward's kept "
                               "state (a second backward through the same graph)")
        # conv -> act -> InstanceNorm (D, U, R.conv1): the bias gradient is the column sum of dt, taken by the pass that writes
        # dt instead of a pass of its own inside the weight gradient (same box, 4 runs: 36.49 / 36.47 against 36.48 / 36.49 ms
        # per step — those column sums ran on the side stream —, -2 GB, -64 launches)
        gb_here = _grad_buffer(bparam) if (want_b and spec.norm and spec.epi_act != ACT_NONE) else None
        dt, dt_amax = block_dt(spec, gp, t, mean, rstd, gb_here)
        if dt is gp:
            dt_amax = _amax_of(g)
        if not dt_amax:
            dt_amax = _measured_amax(dt)      # on this stream, before the weight gradient forks off: both gradients take it
        saved = ctx.saved_state
        # x as the forward saw it?  (autograd refuses a saved tensor that was modified in place, so this only guards a
        # handle that has aged out between forward and backward: measured again below by the library)
        x_amax = ctx.x_amax if (ctx.x_amax and ctx.x_key == (xp._version, xp.data_ptr()) and lib.vcg_amax_valid(ctx.x_amax)) else 0
        if bias_alone and gb_here is not None and GRAD_READY_HOOK[0] is not None:
            GRAD_READY_HOOK[0](None, bparam, torch.cuda.current_stream(dev))
        if run_wgrad:
            # hand the 4x buffer back once the weight gradient has consumed it — not on a traversal that skips the weight
            # gradient (`no_wgrad`: the G phase through a discriminator), whose retained graph is differentiated again
            ctx.saved_state = None
            gw = _grad_buffer(wparam) if want_w else torch.zeros_like(wparam, memory_format=torch.contiguous_format)
            gb = _grad_buffer(bparam) if want_b else None
            if spec.norm and spec.epi_act == ACT_NONE:
                # InstanceNorm directly on conv + bias (CaSb, R.conv2): the mean subtraction cancels the bias, its gradient
                # is identically zero (the reference's autograd returns rounding noise of ~1e-9 there: the column sums of
                # a dt whose columns sum to zero) — the buffer stays at its zeros and the column-sum kernels are not run
                gb = None
            if gb_here is not None:
                gb = None            # already accumulated by block_dt above, on the main stream
            if _OVERLAP[0]:
                side = _side_stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))      # dt (and, the first time, x) are ready
                with torch.cuda.stream(side):
                    conv_wgrad(cd, xp, dt, gw, gb, saved, x_amax, dt_amax, ctx.flops, ctx.tag)
                xp.record_stream(side)                                # the allocator must not recycle them under the side stream
                dt.record_stream(side)
                if saved is not None:
                    saved.record_stream(side)
                if not want_w:
                    gw.record_stream(side)
                wstream = side
            else:
                conv_wgrad(cd, xp, dt, gw, gb, saved, x_amax, dt_amax, ctx.flops, ctx.tag)
                wstream = torch.cuda.current_stream(dev)
            members = getattr(wparam, "_vcg_members", None)
            if members is not None:
                # a fused kernel (FusedConvPair): its gradient was accumulated into scratch; hand the slices to the members'
                # own gradient buffers on the stream the weight gradient ran on, and report THEM to the data-parallel reducer
                # A member that is frozen (or under `no_wgrad`) keeps its `.grad` as it is — None stays None: its slice of the
                # scratch is cleared instead of handed over, so that nothing stale is added once it trains again.
                live = []
                with torch.cuda.stream(wstream):
                    for (mw, mb), (wlo, whi), (blo, bhi) in members:
                        src_w = ctypes.c_void_p(gw.data_ptr() + 4 * wlo)
                        src_b = ctypes.c_void_p(gb.data_ptr() + 4 * blo) if gb is not None and mb is not None else None
                        take_w = mw.requires_grad and id(mw) not in _NO_WGRAD
                        take_b = take_w and src_b is not None and mb.requires_grad
                        if take_w:
                            _native.check(lib.vcg_add_into(_ptr(_grad_buffer(mw)), src_w, whi - wlo, _stream()), "vcg_add_into")
                        else:
                            _native.check(lib.vcg_fill(src_w, 0.0, whi - wlo, _stream()), "vcg_fill")
                        if take_b:
                            _native.check(lib.vcg_add_into(_ptr(_grad_buffer(mb)), src_b, bhi - blo, _stream()), "vcg_add_into")
                        elif src_b is not None:
                            _native.check(lib.vcg_fill(src_b, 0.0, bhi - blo, _stream()), "vcg_fill")
                        if take_w:
                            live.append((mw, mb if take_b else None))
                if GRAD_READY_HOOK[0] is not None:
                    for mw, mb in live:
                        GRAD_READY_HOOK[0](mw, mb, wstream)
            elif GRAD_READY_HOOK[0] is not None:
                if gb_here is not None:      # the bias gradient came from the main stream, the weight gradient from `wstream`
                    GRAD_READY_HOOK[0](None, bparam, torch.cuda.current_stream(dev))
                    GRAD_READY_HOOK[0](wparam, None, wstream)
                else:
                    GRAD_READY_HOOK[0](wparam if want_w else None, bparam, wstream)
        dx = None
        if ctx.needs_input_grad[0] and id(spec) not in _NO_DGRAD:
            dx = logical_of(conv_dgrad(cd, dt, wf, dt_amax, ctx.flops, ctx.tag), spec.cin_phys_log)
        return dx, None, None, d_res, None, None, None, None


def conv_block(x, weight, bias, spec, residual=None, defer=False):
    """`defer`: hand the InstanceNorm's application over to the consumer (see "deferred InstanceNorm" above); only for a
    result whose sole consumer is another conv_block."""
    _require_gpu(x, "conv_block")
    return _ConvBlockFn.apply(x, weight, bias, residual, spec, weight, bias, bool(defer and DEFER_NORM and spec.norm))


# ------------------------------------------------------------------ two convolutions of one input as one (VAE bottleneck: mu and logvar.0)
# False (an A/B run or a test sets the attribute): two separate convolutions, as in round 3
FUSE_MU_LOGVAR = True


class FusedConvPair:
    """Two nn.Conv2d of identical geometry that read the SAME input (reference Networks.py:219-222: muConv and logvarConv[0])
    run as one convolution with the output channels concatenated.  The parameters stay what the reference has (state_dict
    names, optimizer entries); this object keeps a concatenated copy of the weights (refreshed when the members change: one
    device-to-device copy each per optimizer step) and scratch gradient buffers whose slices the backward adds into the
    members' own gradients (`_ConvBlockFn.backward`, `_vcg_members`)."""

    def __init__(self, conv_a, conv_b, spec):
        ca, cb = conv_a.weight.shape[0], conv_b.weight.shape[0]
        if ca % 4 or cb % 4:
            # the split, its adjoint and the hand-over of the gradient slices move float4s (vcg_chan_split, vcg_add_into)
            raise RuntimeError(f"FusedConvPair: both members need a multiple of 4 output channels, got {ca} and {cb}; "
                               "run the two convolutions separately")
        self.a, self.b, self.spec = conv_a, conv_b, spec
        self.w = self.bias = None
        self.key = None
        self.epoch = [0]
        self._written = _WrittenOn()               # where / when the concatenated copy was last refreshed

    def tensors(self):
        wa, wb, ba, bb = self.a.weight, self.b.weight, self.a.bias, self.b.bias
        key = (_param_key(wa), _param_key(wb), _param_key(ba), _param_key(bb), wa.device)
        if self.w is None or self.w.device != wa.device:
            dev = wa.device
            self.w = torch.nn.Parameter(torch.empty((wa.shape[0] + wb.shape[0],) + tuple(wa.shape[1:]), dtype=torch.float32, device=dev))
            self.bias = torch.nn.Parameter(torch.empty(ba.shape[0] + bb.shape[0], dtype=torch.float32, device=dev))
            self.w.grad = torch.zeros_like(self.w)
            self.bias.grad = torch.zeros_like(self.bias)
            self.w._vcg_epoch = self.epoch
            na, nb = wa.numel(), wb.numel()
            self.w._vcg_members = [((wa, ba), (0, na), (0, ba.numel())), ((wb, bb), (na, na + nb), (ba.numel(), ba.numel() + bb.numel()))]
            self.key = None
        if key != self.key:
            with torch.no_grad():
                ca = wa.shape[0]
                self.w.data[:ca].copy_(wa.data)
                self.w.data[ca:].copy_(wb.data)
                self.bias.data[:ca].copy_(ba.data)
                self.bias.data[ca:].copy_(bb.data)
            self.epoch[0] += 1
            self.key = key
            self._written.mark(wa.device)
        else:
            self._written.order_reader(wa.device)      # refreshed by the other direction's chain (DirectionFork)
        rg = wa.requires_grad or wb.requires_grad
        self.w.requires_grad_(rg)
        self.bias.requires_grad_(rg)
        return self.w, self.bias


class _ChanSplitFn(torch.autograd.Function):
    """(N, Ca + Cb, H, W) -> (N, Ca, H, W), (N, Cb, H, W), each its own NHWC tensor."""

    @staticmethod
    def forward(ctx, y, ca):
        yp = as_phys(y)
        n, h, w, c = yp.shape
        cb = c - ca
        a = torch.empty((n, h, w, ca), dtype=torch.float32, device=y.device)
        b = torch.empty((n, h, w, cb), dtype=torch.float32, device=y.device)
        _native.check(_native.lib().vcg_chan_split(_ptr(yp), _ptr(a), _ptr(b), n * h * w, ca, cb, _stream()), "vcg_chan_split")
        ctx.dims = (n, h, w, ca, cb)
        return logical_of(a, ca), logical_of(b, cb)

    @staticmethod
    def backward(ctx, ga, gb):
        n, h, w, ca, cb = ctx.dims
        gap = as_phys(ga) if ga is not None else None
        gbp = as_phys(gb) if gb is not None else None
        dev = (ga if ga is not None else gb).device
        g = torch.empty((n, h, w, ca + cb), dtype=torch.float32, device=dev)
        _native.check(_native.lib().vcg_chan_cat(_ptr(gap), _ptr(gbp), _ptr(g), n * h * w, ca, cb, _stream()), "vcg_chan_cat")
        return logical_of(g, ca + cb), None


def conv_pair(x, pair):
    """Both convolutions of `pair` (a FusedConvPair) applied to x: (y_a, y_b)."""
    _require_gpu(x, "conv_pair")
    w, b = pair.tensors()
    y = _ConvBlockFn.apply(x, w, b, None, pair.spec, w, b, False)
    return _ChanSplitFn.apply(y, pair.a.weight.shape[0])


class _PixelShuffleFn(torch.autograd.Function):
    """nn.PixelShuffle(2) as a standalone copy (used when the producer did not store shuffled)."""

    @staticmethod
    def forward(ctx, x):
        xp = as_phys(x)
        n, h, w, c = xp.shape
        if x.shape[1] != c or c % 16:
            raise RuntimeError(f"pixel_shuffle needs a channel count that is a multiple of 16, got {x.shape[1]}")
        out = torch.empty((n, 2 * h, 2 * w, c // 4), dtype=torch.float32, device=x.device)
        _native.check(_native.lib().vcg_pixel_shuffle(_ptr(xp), _ptr(out), n, h, w, c, 0, _stream()), "vcg_pixel_shuffle")
        ctx.dims = (n, h, w, c)
        return logical_of(out, c // 4)

    @staticmethod
    def backward(ctx, g):
        n, h, w, c = ctx.dims
        gp = as_phys(g)
        dx = torch.empty((n, h, w, c), dtype=torch.float32, device=g.device)
        _native.check(_native.lib().vcg_pixel_shuffle(_ptr(gp), _ptr(dx), n, h, w, c, 1, _stream()), "vcg_pixel_shuffle")
        return logical_of(dx, c)


def pixel_shuffle(x):
    _require_gpu(x, "pixel_shuffle")
    return _PixelShuffleFn.apply(x)


# ------------------------------------------------------------------ VAE sampler
_RNG = {"seed": 0x5EED5EED, "offset": 0}
_EPS_QUEUE = []


def manual_seed(seed):
    """Seed of the on-device Philox stream that draws eps (replaces torch.randn_like, Networks.py:225)."""
    _RNG["seed"] = int(seed) & 0xFFFFFFFFFFFFFFFF
    _RNG["offset"] = 0


RANK_SEED_STRIDE = 7919


def rank_seed(base, rank):
    """Seed of rank `rank`'s eps stream in a data-parallel job whose base seed is `base` (train.py, utils.load_checkpoint)."""
    return (int(base) + RANK_SEED_STRIDE * (int(rank) + 1)) & 0xFFFFFFFFFFFFFFFF


def base_seed_of(seed, rank):
    return (int(seed) - RANK_SEED_STRIDE * (int(rank) + 1)) & 0xFFFFFFFFFFFFFFFF


def inject_eps(tensors):
    """Parity runs: the next reparameterisations consume these eps tensors (NCHW) in call order."""
    _EPS_QUEUE.clear()
    _EPS_QUEUE.extend(tensors)


_TICKETS = []          # draw positions handed out ahead of time (eps_tickets), consumed by the next reparameterisations in call order
_FORCED_OFFSETS = []


def _eps_count(shape):
    """Values one reparameterisation of a logical NCHW `shape` draws: _ReparamFn draws for the PHYSICAL buffer (channel pitch a
    multiple of 4), so a reservation made from the logical count would be too short whenever latent_dim % 4 != 0 and the next
    reserved draw would repeat part of this one."""
    n = 1
    for s in shape:
        n *= s
    return n // shape[1] * pitch(shape[1]) if len(shape) == 4 else n


def eps_tickets(plan, device):
    """Reserve the eps draws of several reparameterisations in the REFERENCE's call order, to be used in another one (the two
    directions of a cycle model are issued interleaved on two streams).  `plan`: [(shape, skip)]; returns one ticket per entry
    (None for skipped ones) for `use_ticket`."""
    del _TICKETS[:], _FORCED_OFFSETS[:]          # leftovers of a forward that raised half way must not shift this one's draws
    out = []
    for shape, skip in plan:
        if _EPS_QUEUE:
            e = _EPS_QUEUE.pop(0)
            if skip:
                out.append(None)
                continue
            if tuple(e.shape) != tuple(shape):
                raise RuntimeError(f"injected eps has shape {tuple(e.shape)}, expected {tuple(shape)}")
            out.append(("tensor", e))
        else:
            n = _eps_count(shape)
            off = _RNG["offset"]
            _RNG["offset"] += (n + 3) // 4
            out.append(None if skip else ("offset", off))
    return out


class use_ticket:
    """The next reparameterisation inside this block draws at the reserved position."""

    def __init__(self, ticket):
        self.ticket = ticket

    def __enter__(self):
        _TICKETS.append(self.ticket)

    def __exit__(self, *exc):
        left = [i for i, t in enumerate(_TICKETS) if t is self.ticket]
        if left:
            del _TICKETS[left[0]]
            if not exc or exc[0] is None:
                raise RuntimeError("an eps ticket was not consumed: the block ran no reparameterisation")
        return False


def next_eps(shape, device, skip=False):
    """Either the next injected eps (as an nhwc view) or None (draw on device).  `skip` consumes
    the stream position of a forward the caller does not compute."""
    if _TICKETS:
        kind, val = _TICKETS.pop(0)
        if skip:
            raise RuntimeError("a reserved eps draw cannot be skipped")
        if kind == "tensor":
            return to_nhwc(val.to(device))
        _FORCED_OFFSETS.append(val)
        return None
    if _EPS_QUEUE:
        e = _EPS_QUEUE.pop(0)
        if skip:
            return None
        if tuple(e.shape) != tuple(shape):
            raise RuntimeError(f"injected eps has shape {tuple(e.shape)}, expected {tuple(shape)}")
        return to_nhwc(e.to(device))
    if skip:
        _RNG["offset"] += (_eps_count(shape) + 3) // 4
    return None


class _ReparamFn(torch.autograd.Function):
    """(mu, logvar_raw) -> (z, clamp(logvar)); Networks.py:223-226."""

    @staticmethod
    def forward(ctx, mu, lv, eps):
        lib = _native.lib()
        mup, lvp = as_phys(mu), as_phys(lv)
        n_el = mup.numel()
        z = torch.empty_like(mup)
        lvc = torch.empty_like(mup)
        if eps is not None:
            epsp = as_phys(eps)
            _native.check(lib.vcg_reparam_fwd(_ptr(mup), _ptr(lvp), _ptr(epsp), None, _ptr(z), _ptr(lvc), n_el, 0, 0,
                                              _stream()), "vcg_reparam_fwd")
        else:
            epsp = torch.empty_like(mup)
            if _FORCED_OFFSETS:
                off = _FORCED_OFFSETS.pop(0)      # reserved by eps_tickets (the counter has already moved past it)
            else:
                off = _RNG["offset"]
                _RNG["offset"] += (n_el + 3) // 4
            _native.check(lib.vcg_reparam_fwd(_ptr(mup), _ptr(lvp), None, _ptr(epsp), _ptr(z), _ptr(lvc), n_el,
                                              _RNG["seed"], off, _stream()), "vcg_reparam_fwd")
        ctx.save_for_backward(epsp, lvp)
        c = mu.shape[1]
        ctx.c_logical = c
        return logical_of(z, c), logical_of(lvc, c)

    @staticmethod
    def backward(ctx, gz, glvc):
        lib = _native.lib()
        epsp, lvp = ctx.saved_tensors
        gzp = as_phys(gz) if gz is not None else None
        glp = as_phys(glvc) if glvc is not None else None
        dmu = torch.empty_like(lvp)
        dlv = torch.empty_like(lvp)
        _native.check(lib.vcg_reparam_bwd(_ptr(gzp), _ptr(glp), _ptr(epsp), _ptr(lvp), _ptr(dmu), _ptr(dlv),
                                          lvp.numel(), _stream()), "vcg_reparam_bwd")
        c = ctx.c_logical            # lvp.shape[3] is the channel PITCH: 8 for latent_dim 6, and autograd refuses that gradient
        return logical_of(dmu, c), logical_of(dlv, c), None


def reparameterize(mu, logvar, eps=None):
    return _ReparamFn.apply(mu, logvar, eps)


# ------------------------------------------------------------------ losses
def _pair_phys(a, b):
    """Two logical NCHW tensors -> physical buffers with identical layout."""
    if a.shape != b.shape:
        raise RuntimeError(f"shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.dim() == 4:
        return as_phys(a), as_phys(b), a.numel()
    _require_gpu(a, "loss")
    _require_gpu(b, "loss")
    return a.contiguous(), b.contiguous(), a.numel()


class _L1Fn(torch.autograd.Function):
    """nn.L1Loss() (mean); Losses.py:21-24."""

    @staticmethod
    def forward(ctx, a, b):
        lib = _native.lib()
        ap, bp, n_log = _pair_phys(a, b)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ws = workspace(lib.vcg_reduce_workspace(ap.numel()), a.device)
        _native.check(lib.vcg_l1_fwd(_ptr(ap), _ptr(bp), _ptr(out), ap.numel(), n_log, _ptr(ws), ws.numel() * 4,
                                     _stream()), "vcg_l1_fwd")
        ctx.save_for_backward(ap, bp)
        ctx.n_log = n_log
        ctx.shape = tuple(a.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _native.lib()
        ap, bp = ctx.saved_tensors
        g = g.contiguous()
        ga = torch.empty_like(ap) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(bp) if ctx.needs_input_grad[1] else None
        if ga is None and gb is None:
            return None, None
        _native.check(lib.vcg_l1_bwd(_ptr(ap), _ptr(bp), _ptr(g), _ptr(ga), _ptr(gb), ap.numel(), ctx.n_log,
                                     _stream()), "vcg_l1_bwd")

        def view(t):
            if t is None:
                return None
            return logical_of(t, ctx.shape[1]) if len(ctx.shape) == 4 else t.view(ctx.shape)
        return view(ga), view(gb)


def l1_loss(a, b):
    return _L1Fn.apply(a, b)


def _call(entry, *args):
    """lib.<entry>(*args), the entry looked up when it is called, its status checked."""
    _native.check(getattr(_native.lib(), entry)(*args), entry)


def _scratch(entry, *args):
    """The byte count lib.<entry>(*args) asks for; 0 means the library refused the arguments."""
    need = getattr(_native.lib(), entry)(*args)
    if need == 0:
        _native.check(-1, entry)
    return need


# The optional image losses differ in their library calls, their one option `opt` and what the backward reads; _ImageLossFn holds
# everything else.  scratch(n, h, w, opt) -> workspace bytes; fwd(ap, bp, out, dims, opt, ws) -> the tensors kept for the backward;
# bwd(kept, g, ga, dims, opt).
class _SsimTerm:
    """1 - mean SSIM(generated, target) (csrc/ssim_loss.hip)."""
    name = "ssim_loss"

    @staticmethod
    def scratch(n, h, w, _):
        return _scratch("vcg_ssim_loss_workspace", n, h, w)

    @staticmethod
    def fwd(ap, bp, out, dims, _, ws):
        _call("vcg_ssim_loss_fwd", _ptr(ap), _ptr(bp), _ptr(out), *dims, _ptr(ws), ws.numel() * 4, _stream())
        return ap, bp                             # the backward recomputes its coefficients from the two images

    @staticmethod
    def bwd(kept, g, ga, dims, _):
        ap, bp = kept
        _call("vcg_ssim_loss_bwd", _ptr(ap), _ptr(bp), _ptr(g), _ptr(ga), *dims, _stream())


class _MsssimTerm:
    """1 - mean MS-SSIM(generated, target) (csrc/msssim_loss.hip); opt: the number of scales.  The forward keeps its workspace —
    the pooled levels and the table d loss / d factor — for the backward, so none of it lives in the shared scratch buffer."""
    name = "msssim_loss"

    @staticmethod
    def scratch(n, h, w, scales):
        return 0

    @staticmethod
    def fwd(ap, bp, out, dims, scales, _):
        keep = torch.empty(_scratch("vcg_msssim_loss_workspace", *dims, scales) // 4, dtype=torch.float32, device=ap.device)
        _call("vcg_msssim_loss_fwd", _ptr(ap), _ptr(bp), _ptr(out), *dims, scales, _ptr(keep), keep.numel() * 4, _stream())
        return ap, bp, keep

    @staticmethod
    def bwd(kept, g, ga, dims, scales):
        ap, bp, keep = kept
        _call("vcg_msssim_loss_bwd", _ptr(ap), _ptr(bp), _ptr(g), _ptr(ga), *dims, scales, _ptr(keep), keep.numel() * 4, _stream())


class _GradTerm:
    """Multi-scale gradient-matching loss of (generated, target) (csrc/grad_loss.hip); opt: the number of scales."""
    name = "grad_match_loss"

    @staticmethod
    def scratch(n, h, w, scales):
        return _scratch("vcg_grad_loss_workspace", n, h, w, scales)

    @staticmethod
    def fwd(ap, bp, out, dims, scales, ws):
        _call("vcg_grad_loss_fwd", _ptr(ap), _ptr(bp), _ptr(out), *dims, scales, _ptr(ws), ws.numel() * 4, _stream())
        return ap, bp                             # the backward takes its signs from the two images

    @staticmethod
    def bwd(kept, g, ga, dims, scales):
        ap, bp = kept
        _call("vcg_grad_loss_bwd", _ptr(ap), _ptr(bp), _ptr(g), _ptr(ga), *dims, scales, _stream())


class _FreqTerm:
    """Focal frequency loss of (generated, target) (csrc/freq_loss.hip); opt: alpha.  The forward keeps the spectrum of
    generated - target and the plane maxima; the backward reads those, not the images."""
    name = "freq_loss"

    @staticmethod
    def scratch(n, h, w, _):
        return _scratch("vcg_freq_loss_workspace", n, h, w)

    @staticmethod
    def fwd(ap, bp, out, dims, alpha, ws):
        keep = _scratch("vcg_freq_loss_spectrum", *dims)
        spec = torch.empty(keep // 4, dtype=torch.float32, device=ap.device)
        _call("vcg_freq_loss_fwd", _ptr(ap), _ptr(bp), _ptr(out), *dims, alpha, _ptr(spec), keep, _ptr(ws), ws.numel() * 4, _stream())
        return (spec,)

    @staticmethod
    def bwd(kept, g, ga, dims, alpha):
        spec, = kept
        ws = workspace(_FreqTerm.scratch(*dims, alpha), spec.device)
        _call("vcg_freq_loss_bwd", _ptr(spec), spec.numel() * 4, _ptr(g), _ptr(ga), *dims, alpha, _ptr(ws), ws.numel() * 4, _stream())


class _ImageLossFn(torch.autograd.Function):
    """The loss `term` (_SsimTerm, _MsssimTerm, _GradTerm, _FreqTerm) of (generated, target); the gradient reaches `generated` only."""

    @staticmethod
    def forward(ctx, term, a, b, opt):
        if a.shape != b.shape:
            raise RuntimeError(f"{term.name}: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
        if a.dim() != 4 or a.shape[1] != 3:
            raise RuntimeError(f"{term.name}: expected (N, 3, H, W) images, got shape {tuple(a.shape)}")
        ap, bp = as_phys(a), as_phys(b)
        dims = tuple(ap.shape[:3])
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ws = workspace(term.scratch(*dims, opt), a.device)
        ctx.save_for_backward(*term.fwd(ap, bp, out, dims, opt, ws))
        ctx.call = (term, dims, opt)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        term, dims, opt = ctx.call
        g = g.contiguous()
        ga = torch.empty((*dims, 4), dtype=torch.float32, device=g.device)
        term.bwd(ctx.saved_tensors, g, ga, dims, opt)
        return None, logical_of(ga, 3), None, None


def _image_loss(term, generated, target, opt=None):
    if target.requires_grad:
        raise RuntimeError(f"{term.name}: the target must not require a gradient (only d loss / d generated is computed)")
    return _ImageLossFn.apply(term, generated, target, opt)


def ssim_loss(generated, target):
    """1 - mean SSIM over (N, 3, H, W) images, H, W >= 11: a 0-dim fp32 tensor.  `target` is an input image: no gradient."""
    return _image_loss(_SsimTerm, generated, target)


MSSSIM_MAX_SCALES = 5
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)         # Wang, Simoncelli & Bovik 2003; the first K over their sum


def msssim_weights(scales):
    """The exponents of the `scales` levels of `msssim_loss`: they sum to 1."""
    total = sum(MSSSIM_WEIGHTS[:scales])
    return tuple(w / total for w in MSSSIM_WEIGHTS[:scales])


def msssim_max_scales(h, w):
    """The largest `scales` in 0..5 that `msssim_loss` accepts for H x W images: the coarsest level, min(H, W) >> (scales - 1),
    must still hold the 11 x 11 window.  0: not even one scale.  Host arithmetic only."""
    k = 0
    while k < MSSSIM_MAX_SCALES and (min(int(h), int(w)) >> k) >= 11:
        k += 1
    return k


def msssim_loss(generated, target, scales=5):
    """1 - mean over images and channels of MS-SSIM (the product over `scales` in 1..5 levels of a 2 x 2 mean pyramid of the
    mean contrast-structure, the coarsest level's mean SSIM, each clamped below at 1e-4 and raised to its weight) of (N, 3, H, W)
    images, min(H, W) >> (scales - 1) >= 11: a 0-dim fp32 tensor.  scales = 1 is `ssim_loss`.  `target` is an input image: no
    gradient."""
    if isinstance(scales, bool) or int(scales) != scales or not 1 <= int(scales) <= MSSSIM_MAX_SCALES:
        raise RuntimeError(f"msssim_loss: scales must be an integer in 1..{MSSSIM_MAX_SCALES}, got {scales!r}")
    return _image_loss(_MsssimTerm, generated, target, int(scales))


def grad_match_loss(generated, target, scales=4):
    """Mean |horizontal and vertical finite differences of generated - target| over `scales` in 1..4 subsampled scales of
    (N, 3, H, W) images, H, W >= 1: a 0-dim fp32 tensor.  `target` is an input image: no gradient."""
    if isinstance(scales, bool) or int(scales) != scales or not 1 <= int(scales) <= 4:
        raise RuntimeError(f"grad_match_loss: scales must be an integer in 1..4, got {scales!r}")
    return _image_loss(_GradTerm, generated, target, int(scales))


def freq_loss(generated, target, alpha=1.0):
    """Focal frequency loss (Jiang et al. 2021) of (N, 3, H, W) images, H, W in 1..2048: the mean over planes and frequencies of
    w |D|^2, D the orthonormal 2-D DFT of generated - target and w = |D|^alpha over its plane maximum, a constant for the
    gradient: a 0-dim fp32 tensor.  `target` is an input image: no gradient."""
    alpha = float(alpha)
    if not math.isfinite(alpha) or alpha < 0.0:
        raise RuntimeError(f"freq_loss: alpha must be finite and >= 0, got {alpha!r}")
    return _image_loss(_FreqTerm, generated, target, alpha)


class _MseConstFn(torch.autograd.Function):
    """nn.MSELoss()(d, full_like(d, target)) and d.mean(); Losses.py:80-81,99-100, Networks.py:2048-2051."""

    @staticmethod
    def forward(ctx, d, target):
        lib = _native.lib()
        _require_gpu(d, "mse_const")
        dc = d.contiguous()
        out = torch.empty(2, dtype=torch.float32, device=d.device)
        _native.check(lib.vcg_mse_const_fwd(_ptr(dc), float(target), _ptr(out), dc.numel(), _stream()), "vcg_mse_const_fwd")
        ctx.save_for_backward(dc)
        ctx.target = float(target)
        loss, mean = out[0], out[1]
        ctx.mark_non_differentiable(mean)
        return loss, mean

    @staticmethod
    def backward(ctx, g, _gmean):
        lib = _native.lib()
        (dc,) = ctx.saved_tensors
        g = g.contiguous()
        gd = torch.empty_like(dc)
        _native.check(lib.vcg_mse_const_bwd(_ptr(dc), ctx.target, _ptr(g), _ptr(gd), dc.numel(), _stream()), "vcg_mse_const_bwd")
        return gd, None


def mse_const(d, target):
    """-> (mean((d-target)^2), mean(d))"""
    return _MseConstFn.apply(d, target)


GAN_OBJECTIVES = ("lsgan", "hinge", "logistic")      # the index is the library's VCG_GAN_* code


def _dense_logits(t, what):
    if t is None:
        return None
    _require_gpu(t, what)
    if t.numel() == 0:
        raise RuntimeError(f"{what}: empty logit tensor of shape {tuple(t.shape)}")
    return t.contiguous()


class _GanTermsFn(torch.autograd.Function):
    """The six adversarial scalars of one discriminator's (real, fake) logits (csrc/gan_terms.hip): one launch forward, one
    backward per phase of the step.  A side without an upstream gradient gets None, so autograd does not walk its discriminator
    pass: VAEGAN's D phase (the real term alone) and the generator phase (the fake terms alone) cost what they do under LSGAN."""

    @staticmethod
    def forward(ctx, real, fake, code, smooth):
        rc, fc = _dense_logits(real, "gan_terms"), _dense_logits(fake, "gan_terms")
        dev = (rc if rc is not None else fc).device
        out = torch.empty(6, dtype=torch.float32, device=dev)
        _call("vcg_gan_terms_fwd", _ptr(rc), 0 if rc is None else rc.numel(), _ptr(fc), 0 if fc is None else fc.numel(),
              code, smooth, _ptr(out), _stream())
        ctx.sides = (rc is not None, fc is not None)
        ctx.save_for_backward(*[t for t in (rc, fc) if t is not None])
        ctx.call = (code, smooth)
        ctx.set_materialize_grads(False)
        terms = tuple(out[i] for i in range(6))
        ctx.mark_non_differentiable(terms[4], terms[5])
        return terms

    @staticmethod
    def backward(ctx, g_g_real, g_g_fake, g_d_real, g_d_fake, _g_mean_real, _g_mean_fake):
        if torch.is_grad_enabled():               # create_graph=True: a gradient penalty or the like wants d/dz of this result
            raise RuntimeError("gan_terms: the gradient cannot be differentiated a second time (create_graph=True); "
                               "the op has a first derivative only")
        saved = list(ctx.saved_tensors)
        rc = saved.pop(0) if ctx.sides[0] else None
        fc = saved.pop(0) if ctx.sides[1] else None
        code, smooth = ctx.call
        ups = [None if g is None else g.contiguous() for g in (g_g_real, g_g_fake, g_d_real, g_d_fake)]
        # a side takes part when it is present, wanted, and one of its two terms is differentiated
        if rc is None or not ctx.needs_input_grad[0] or (ups[0] is None and ups[2] is None):
            rc, ups[0], ups[2] = None, None, None
        if fc is None or not ctx.needs_input_grad[1] or (ups[1] is None and ups[3] is None):
            fc, ups[1], ups[3] = None, None, None
        if rc is None and fc is None:
            return None, None, None, None
        g_real = None if rc is None else torch.empty_like(rc)
        g_fake = None if fc is None else torch.empty_like(fc)
        table = (ctypes.c_void_p * 4)(*[None if g is None else g.data_ptr() for g in ups])
        _call("vcg_gan_terms_bwd", _ptr(rc), 0 if rc is None else rc.numel(), _ptr(fc), 0 if fc is None else fc.numel(),
              code, smooth, table, _ptr(g_real), _ptr(g_fake), _stream())
        return g_real, g_fake, None, None


def gan_terms(real, fake, objective, smooth=0.0):
    """-> (g_real, g_fake, d_real, d_fake, mean_real, mean_fake), 0-dim fp32 tensors: the generator's and the discriminator's
    adversarial terms on a discriminator's logits of real and of generated images, and the logit means.  `objective` is one of
    GAN_OBJECTIVES; with s = `smooth` (one-sided label smoothing, 0 <= s < 0.5, 0 with the hinge) and
    sp(t) = max(t, 0) + log1p(exp(-|t|)), each term is the mean over its tensor of

        objective   d_real                      d_fake          g_real   g_fake
        lsgan       (z - (1 - s))^2             z^2             z^2      (z - 1)^2
        hinge       max(0, 1 - z)               max(0, 1 + z)   z        -z
        logistic    (1 - s) sp(-z) + s sp(z)    sp(z)           sp(z)    sp(-z)

    evaluated and summed in double and rounded once.  `real` or `fake` may be None (not both): its three results are 0 and carry no
    gradient.  The four terms are differentiable once in the logits; the means carry no gradient."""
    if objective not in GAN_OBJECTIVES:
        raise RuntimeError(f"gan_terms: objective must be one of {GAN_OBJECTIVES}, got {objective!r}")
    if isinstance(smooth, bool) or not isinstance(smooth, (int, float)) or not math.isfinite(smooth) or not 0.0 <= smooth < 0.5:
        raise RuntimeError(f"gan_terms: smooth must be a finite number in [0, 0.5), got {smooth!r}")
    if objective == "hinge" and smooth != 0.0:
        raise RuntimeError(f"gan_terms: the hinge objective takes no label smoothing, got smooth={smooth!r}")
    if real is None and fake is None:
        raise RuntimeError("gan_terms: real and fake are both None")
    return _GanTermsFn.apply(real, fake, GAN_OBJECTIVES.index(objective), float(smooth))


FM_MODES = ("pair", "mean")                          # the index is the library's VCG_FM_* code
FM_MAX_LAYERS = 4                                    # VCG_FM_MAX_LAYERS


def fm_chunk(mode, channels=4):
    """The work one workgroup of the feature-matching kernels takes at a time (vcg_feature_match_chunk): float4s of a layer per
    chunk in the pair mode — rows, for a layer of 1..4 channels —, rows per slab of a layer with `channels` channels in the mean
    mode.  The sizes at which the kernels change path; the tests place their shapes around them."""
    if mode not in FM_MODES:
        raise RuntimeError(f"fm_chunk: mode must be one of {FM_MODES}, got {mode!r}")
    return _scratch("vcg_feature_match_chunk", FM_MODES.index(mode), int(channels))


class _FeatureMatchFn(torch.autograd.Function):
    """The feature-matching term of up to four (generated, real) activation pairs (csrc/feature_match.hip): two launches forward
    (three in the mean mode), one backward, each for all layers.  The real side is a constant: its inputs get None, so autograd does not walk the real pass."""

    @staticmethod
    def forward(ctx, code, n, *tensors):
        fakes, reals = tensors[:n], tensors[n:]
        fp, rp = [as_phys(t) for t in fakes], [as_phys(t) for t in reals]
        dev = fakes[0].device
        rows = (ctypes.c_size_t * n)(*[p.shape[0] * p.shape[1] * p.shape[2] for p in fp])
        chans = (ctypes.c_int * n)(*[t.shape[1] for t in fakes])
        out = torch.empty((), dtype=torch.float32, device=dev)
        signs = torch.empty(sum(pitch(t.shape[1]) for t in fakes), dtype=torch.float32, device=dev) if code == 1 else None
        ws = workspace(_scratch("vcg_feature_match_workspace", rows, chans, n, code), dev)
        _call("vcg_feature_match_fwd", (ctypes.c_void_p * n)(*[p.data_ptr() for p in fp]),
              (ctypes.c_void_p * n)(*[p.data_ptr() for p in rp]), rows, chans, n, code, _ptr(out), _ptr(signs), _ptr(ws),
              ws.numel() * 4, _stream())
        # pair: the sign is recomputed from the operands; mean: the channel signs stand for both
        ctx.save_for_backward(*(fp + rp if code == 0 else [signs]))
        ctx.call = (code, n, [tuple(t.shape) for t in fakes])
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():               # create_graph=True
            raise RuntimeError("feature_matching: the gradient cannot be differentiated a second time (create_graph=True); "
                               "the op has a first derivative only")
        code, n, shapes = ctx.call
        wanted = [ctx.needs_input_grad[2 + i] for i in range(n)]
        if not any(wanted):
            return (None,) * (2 + 2 * n)
        saved = ctx.saved_tensors
        fp, rp, signs = (saved[:n], saved[n:], None) if code == 0 else (None, None, saved[0])
        g = g.contiguous()
        dev = g.device
        grads = [torch.empty((s[0], s[2], s[3], pitch(s[1])), dtype=torch.float32, device=dev) if w else None
                 for s, w in zip(shapes, wanted)]

        def table(ts):
            return (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
        rows = (ctypes.c_size_t * n)(*[s[0] * s[2] * s[3] for s in shapes])
        chans = (ctypes.c_int * n)(*[s[1] for s in shapes])
        _call("vcg_feature_match_bwd", None if fp is None else table(fp), None if rp is None else table(rp), _ptr(signs), _ptr(g),
              table(grads), rows, chans, n, code, _stream())
        return (None, None, *[None if t is None else logical_of(t, s[1]) for t, s in zip(grads, shapes)], *([None] * n))


def feature_matching(fakes, reals, mode):
    """The discriminator feature-matching term -> a 0-dim fp32 tensor.  `fakes`, `reals`: sequences of 1..4 logical (N, C, H, W)
    activations with equal shapes pairwise — a discriminator's block outputs on the generated and on the real batch.  With L layers,
    fm = (1 / L) sum_l term_l and `mode` one of FM_MODES:

        pair   term_l = mean over all elements of |f_l - r_l|                       (pix2pixHD; image i of the fakes belongs to image i of
                                                                                     the reals)
        mean   term_l = (1 / C_l) sum_c |mean_{n,h,w} f_l[:, c] - mean_{n,h,w} r_l[:, c]|   (Salimans et al. 2016; needs no pairing)

    summed in double and rounded once.  The reals are constants of the term: it is differentiable once in each fake, with
    sign(0) = 0, and every real gets None."""
    for name, seq in (("fakes", fakes), ("reals", reals)):
        if not isinstance(seq, (list, tuple)):
            raise RuntimeError(f"feature_matching: {name} must be a list or tuple of tensors, got {type(seq).__name__}")
        if not 1 <= len(seq) <= FM_MAX_LAYERS:
            raise RuntimeError(f"feature_matching: {name} must hold 1..{FM_MAX_LAYERS} layers, got {len(seq)}")
        for i, t in enumerate(seq):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError(f"feature_matching: {name}[{i}] is not a tensor but {type(t).__name__}")
            if t.dim() != 4:
                raise RuntimeError(f"feature_matching: {name}[{i}] must be an (N, C, H, W) tensor, got shape {tuple(t.shape)}")
            if t.numel() == 0:
                raise RuntimeError(f"feature_matching: {name}[{i}] is empty, shape {tuple(t.shape)}")
            if t.dtype != torch.float32:
                raise RuntimeError(f"feature_matching: {name}[{i}]: expected float32, got {t.dtype}")
    if len(fakes) != len(reals):
        raise RuntimeError(f"feature_matching: fakes has {len(fakes)} layers, reals {len(reals)}")
    for i, (f, r) in enumerate(zip(fakes, reals)):
        if f.shape != r.shape:
            raise RuntimeError(f"feature_matching: fakes[{i}] has shape {tuple(f.shape)}, reals[{i}] {tuple(r.shape)}")
    if mode not in FM_MODES:
        raise RuntimeError(f"feature_matching: mode must be one of {FM_MODES}, got {mode!r}")
    for name, seq in (("fakes", fakes), ("reals", reals)):
        for i, t in enumerate(seq):
            _require_gpu(t, f"feature_matching: {name}[{i}]")
    return _FeatureMatchFn.apply(FM_MODES.index(mode), len(fakes), *fakes, *reals)


class _KLFn(torch.autograd.Function):
    """KLDivergenceLoss.forward; Losses.py:115-121."""

    @staticmethod
    def forward(ctx, mu, lv):
        lib = _native.lib()
        # vcg_kl_fwd / vcg_kl_bwd take the mean over the n values they are handed: the physical buffers serve only where they hold
        # nothing but the logical values.  A latent with pad lanes (latent_dim % 4 != 0: 6 lives at pitch 8) goes in as a dense
        # copy — over the physical buffer the sum is the same (a pad lane adds 1 + 0 - 0 - e^0 = 0) but the mean is 6/8 of it.
        ctx.phys = mu.dim() == 4 and pitch(mu.shape[1]) == mu.shape[1]
        if ctx.phys:
            mup, lvp, _ = _pair_phys(mu, lv)
        else:
            if mu.shape != lv.shape:
                raise RuntimeError(f"shape mismatch {tuple(mu.shape)} vs {tuple(lv.shape)}")
            _require_gpu(mu, "loss")
            _require_gpu(lv, "loss")
            mup, lvp = mu.contiguous(), lv.contiguous()
        out = torch.empty((), dtype=torch.float32, device=mu.device)
        ws = workspace(lib.vcg_reduce_workspace(mup.numel()), mu.device)
        _native.check(lib.vcg_kl_fwd(_ptr(mup), _ptr(lvp), _ptr(out), mup.numel(), _ptr(ws), ws.numel() * 4, _stream()), "vcg_kl_fwd")
        ctx.save_for_backward(mup, lvp)
        ctx.shape = tuple(mu.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _native.lib()
        mup, lvp = ctx.saved_tensors
        g = g.contiguous()
        gmu = torch.empty_like(mup)
        glv = torch.empty_like(lvp)
        _native.check(lib.vcg_kl_bwd(_ptr(mup), _ptr(lvp), _ptr(g), _ptr(gmu), _ptr(glv), mup.numel(), _stream()), "vcg_kl_bwd")
        if ctx.phys:
            return logical_of(gmu, ctx.shape[1]), logical_of(glv, ctx.shape[1])
        return gmu.view(ctx.shape), glv.view(ctx.shape)


def kl_loss(mu, logvar):
    return _KLFn.apply(mu, logvar)


def _kl_fb_phys(t):
    """mu or logvar of `kl_free_bits` -> its physical (N, h, w, pitch(C)) buffer: an (N, C, h, w) latent of the networks in place
    (pad lanes included: the kernels never sum them), anything else — a 2-D (N, C) tensor as (N, C, 1, 1), another layout, a
    tensor whose pad lanes are not the package's — through the dense copy `as_phys` makes."""
    if t.dim() == 2:
        t = t.reshape(t.shape[0], t.shape[1], 1, 1)
    elif t.dim() != 4:
        raise RuntimeError(f"kl_free_bits: expected an (N, C, h, w) or (N, C) latent, got shape {tuple(t.shape)}")
    if t.numel() == 0:
        raise RuntimeError(f"kl_free_bits: empty latent of shape {tuple(t.shape)}")
    return as_phys(t)


class _KLFreeBitsFn(torch.autograd.Function):
    """KLDivergenceLoss.forward (Losses.py:115-121) with a free-bits floor per channel (csrc/kl_free_bits.hip) ->
    (floored mean, plain mean, open gates, the (C,) channel KLs); the gradient reaches mu and logvar through the floored mean only."""

    @staticmethod
    def forward(ctx, mu, lv, floor):
        if mu.shape != lv.shape:
            raise RuntimeError(f"shape mismatch {tuple(mu.shape)} vs {tuple(lv.shape)}")
        mup, lvp = _kl_fb_phys(mu), _kl_fb_phys(lv)
        n, h, w, cp = mup.shape
        rows, c = n * h * w, mu.shape[1]
        out = torch.empty(3, dtype=torch.float32, device=mu.device)
        klc = torch.empty(c, dtype=torch.float32, device=mu.device)
        ws = workspace(_scratch("vcg_kl_fb_workspace", rows, cp), mu.device)
        _call("vcg_kl_fb_fwd", _ptr(mup), _ptr(lvp), _ptr(out), _ptr(klc), rows, c, cp, floor, _ptr(ws), ws.numel() * 4, _stream())
        ctx.save_for_backward(mup, lvp, klc)
        ctx.call = (rows, c, cp, floor, tuple(mu.shape))
        loss, plain, active = out[0], out[1], out[2]
        ctx.mark_non_differentiable(plain, active, klc)
        return loss, plain, active, klc

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gplain, _gactive, _gklc):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        mup, lvp, klc = ctx.saved_tensors
        rows, c, cp, floor, shape = ctx.call
        g = g.contiguous()
        gmu, glv = torch.empty_like(mup), torch.empty_like(lvp)
        _call("vcg_kl_fb_bwd", _ptr(mup), _ptr(lvp), _ptr(g), _ptr(klc), _ptr(gmu), _ptr(glv), rows, c, cp, floor, _stream())

        def view(t, wanted):
            if not wanted:
                return None
            t = logical_of(t, c)
            return t if len(shape) == 4 else t.reshape(shape)
        return view(gmu, ctx.needs_input_grad[0]), view(glv, ctx.needs_input_grad[1]), None


def kl_free_bits(mu, logvar, floor, channel_kl=False):
    """The KL term with a free-bits floor (Kingma et al. 2016) -> (loss, plain, active), 0-dim fp32 tensors.  With KL_c the mean
    over batch and positions of -0.5 (1 + l - mu^2 - exp(l)), l = clamp(logvar, -10, 10), of channel c (dimension 1):
    loss = mean_c max(KL_c, floor), differentiable once in mu and logvar — a channel at or below the floor passes no gradient;
    plain = mean_c KL_c, `kl_loss`'s value; active = the number of channels above the floor.  plain and active carry no
    gradient.  channel_kl=True appends the (C,) tensor of the KL_c."""
    floor = float(floor)
    if not math.isfinite(floor) or floor < 0.0:
        raise RuntimeError(f"kl_free_bits: the floor must be finite and >= 0, got {floor!r}")
    _require_gpu(mu, "kl_free_bits")
    _require_gpu(logvar, "kl_free_bits")
    out = _KLFreeBitsFn.apply(mu, logvar, floor)
    return out if channel_kl else out[:3]


class _LinCombFn(torch.autograd.Function):
    """sum_i w_i * s_i over scalar device tensors (the composite-loss lines Networks.py:941, 2012-2018)."""

    @staticmethod
    def forward(ctx, weights, *terms):
        lib = _native.lib()
        k = len(terms)
        ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in terms])
        ws = (ctypes.c_float * k)(*[float(w) for w in weights])
        out = torch.empty((), dtype=torch.float32, device=terms[0].device)
        _native.check(lib.vcg_lincomb_fwd(ptrs, ws, k, _ptr(out), _stream()), "vcg_lincomb_fwd")
        ctx.weights = [float(w) for w in weights]
        ctx.keep = terms  # keep the scalars alive until the kernel has run
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _native.lib()
        outs = []
        for w in ctx.weights:
            o = torch.empty((), dtype=torch.float32, device=g.device)
            ptrs = (ctypes.c_void_p * 1)(g.data_ptr())
            ws = (ctypes.c_float * 1)(w)
            _native.check(lib.vcg_lincomb_fwd(ptrs, ws, 1, _ptr(o), _stream()), "vcg_lincomb_fwd")
            outs.append(o)
        return (None, *outs)


def weighted_sum(terms, weights):
    terms = [t for t in terms]
    for t in terms:
        _require_gpu(t, "weighted_sum")
    return _LinCombFn.apply(list(weights), *terms)


# ------------------------------------------------------------------ spectral-normed discriminator head
HEAD_STRIDE = 16    # the discriminator body halves the image four times before the head (Networks.py:241-247)


def head_output_shape(image_h, image_w=None, kernel=(16, 16)):
    """(OH, OW) of the discriminator head's logits for an image of image_h x image_w pixels (square when image_w is None): the
    body's four stride-2 layers leave a map of image / 16, and the head is a valid, stride-1 convolution over it
    (Networks.py:248) — (1, 1) at 256 x 256, (17, 17) at 512 x 512.  Raises for a size the head does not accept."""
    image_w = image_h if image_w is None else image_w
    kh, kw = kernel
    for side in (image_h, image_w):
        if int(side) != side or side % HEAD_STRIDE:
            raise RuntimeError(f"discriminator image sizes must be multiples of {HEAD_STRIDE}; got {image_h}x{image_w}")
    h, w = int(image_h) // HEAD_STRIDE, int(image_w) // HEAD_STRIDE
    if h < kh or w < kw:
        raise RuntimeError(_head_too_small(h, w, kh, kw))
    return h - kh + 1, w - kw + 1


def _head_too_small(h, w, kh, kw, c=None):
    what = f"{h}x{w}" if c is None else f"{c}x{h}x{w}"
    return (f"discriminator head: a {what} map is smaller than the {kh}x{kw} kernel; the smallest accepted image is "
            f"{HEAD_STRIDE * kh}x{HEAD_STRIDE * kw} (the reference's Conv2d(512, 1, 16, padding=0) fails below it too)")


class _FullMapSNFn(torch.autograd.Function):
    """spectral_norm(nn.Conv2d(C, 1, k, padding=0)) followed by .view(-1, 1).squeeze(1) -> (N OH OW,)  (Networks.py:248, :269).
    A k x k map (256 x 256 images) is one dot product per image, the vcg_fullmap_* kernels; a larger map is the sliding
    (patch) convolution of the vcg_patch_head_* kernels.  The spectral-norm state is handled the same way for both."""

    @staticmethod
    def forward(ctx, x, weight_orig, bias, u, v, training, wparam, bparam):
        lib = _native.lib()
        xp = as_phys(x)
        n, h, w, c = xp.shape
        _, cw, kh, kw = weight_orig.shape
        if c != cw:
            raise RuntimeError(f"discriminator head expects {cw} channels; got a {c}x{h}x{w} map")
        if h < kh or w < kw:
            raise RuntimeError(_head_too_small(h, w, kh, kw, c))
        dev = x.device
        k = c * kh * kw
        patch = (h, w) != (kh, kw)
        if patch:
            ws_bytes = lib.vcg_patch_head_workspace(n, h, w, c, kh, kw)
            if not ws_bytes:
                _native.check(-1, "vcg_patch_head_workspace")
        sigma = torch.empty(1, dtype=torch.float32, device=dev)
        wsn = torch.empty(k, dtype=torch.float32, device=dev)
        wo = weight_orig.detach().contiguous()
        ws = workspace(64, dev)
        _native.check(lib.vcg_sn_prepare(_ptr(wo), _ptr(u), _ptr(v), _ptr(sigma), _ptr(wsn), c, kh, kw, int(training),
                                         _ptr(ws), 64, _stream()), "vcg_sn_prepare")
        if patch:
            out = torch.empty(n * (h - kh + 1) * (w - kw + 1), dtype=torch.float32, device=dev)
            ws = workspace(ws_bytes, dev)
            _native.check(lib.vcg_patch_head_fwd(_ptr(xp), _ptr(wsn), _ptr(bias), _ptr(out), n, h, w, c, kh, kw, _ptr(ws),
                                                 ws.numel() * 4, _stream()), "vcg_patch_head_fwd")
        else:
            out = torch.empty(n, dtype=torch.float32, device=dev)
            _native.check(lib.vcg_fullmap_fwd(_ptr(xp), _ptr(wsn), _ptr(bias), _ptr(out), n, k, _stream()), "vcg_fullmap_fwd")
        ctx.save_for_backward(xp, wsn, sigma, u.clone(), v.clone())
        ctx.dims = (n, h, w, c, kh, kw)
        ctx.wparam, ctx.bparam = wparam, bparam
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _native.lib()
        xp, wsn, sigma, u, v = ctx.saved_tensors
        n, h, w, c, kh, kw = ctx.dims
        k = c * kh * kw
        patch = (h, w) != (kh, kw)
        g = g.contiguous()
        dev = g.device
        wparam, bparam = ctx.wparam, ctx.bparam
        want_w = wparam is not None and wparam.requires_grad and id(wparam) not in _NO_WGRAD
        # a trainable bias under a frozen weight: the same kernel, its weight part into scratch that is dropped
        bias_alone = (not want_w and wparam is not None and not wparam.requires_grad and bparam is not None
                      and bparam.requires_grad and id(bparam) not in _NO_WGRAD)
        if want_w or bias_alone:
            gw = _grad_buffer(wparam) if want_w else torch.zeros_like(wparam, memory_format=torch.contiguous_format)
            gb = _grad_buffer(bparam) if (bparam is not None and bparam.requires_grad) else None
            if patch:
                ws = workspace(lib.vcg_patch_head_workspace(n, h, w, c, kh, kw), dev)
                _native.check(lib.vcg_patch_head_wgrad(_ptr(g), _ptr(xp), _ptr(wsn), _ptr(sigma), _ptr(u), _ptr(v), _ptr(gw),
                                                       _ptr(gb), n, h, w, c, kh, kw, _ptr(ws), ws.numel() * 4, _stream()),
                              "vcg_patch_head_wgrad")
            else:
                ws = workspace((k + 256) * 4, dev)
                _native.check(lib.vcg_fullmap_wgrad(_ptr(g), _ptr(xp), _ptr(wsn), _ptr(sigma), _ptr(u), _ptr(v), _ptr(gw),
                                                    _ptr(gb), n, c, kh, kw, _ptr(ws), ws.numel() * 4, _stream()), "vcg_fullmap_wgrad")
            if GRAD_READY_HOOK[0] is not None:
                GRAD_READY_HOOK[0](wparam if want_w else None, bparam, torch.cuda.current_stream(dev))
        dx = None
        if ctx.needs_input_grad[0]:
            dxp = torch.empty_like(xp)
            if patch:
                _native.check(lib.vcg_patch_head_dgrad(_ptr(g), _ptr(wsn), _ptr(dxp), n, h, w, c, kh, kw, _stream()),
                              "vcg_patch_head_dgrad")
            else:
                _native.check(lib.vcg_fullmap_dgrad(_ptr(g), _ptr(wsn), _ptr(dxp), n, k, _stream()), "vcg_fullmap_dgrad")
            dx = logical_of(dxp, c)
        return dx, None, None, None, None, None, None, None


def fullmap_sn_conv(x, weight_orig, bias, u, v, training):
    """The discriminator head on an NHWC map of at least the kernel's size -> logits (N OH OW,), n-major, then oy, then ox."""
    _require_gpu(x, "fullmap_sn_conv")
    return _FullMapSNFn.apply(x, weight_orig, bias, u, v, training, weight_orig, bias)


# ------------------------------------------------------------------ misc
def fill_(t, value=0.0):
    _require_gpu(t, "fill_")
    if not t.is_contiguous():
        raise RuntimeError("fill_: tensor must be contiguous")
    _native.check(_native.lib().vcg_fill(_ptr(t), float(value), t.numel(), _stream()), "vcg_fill")
    return t


def randn(shape, device, seed, offset=0):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _native.check(_native.lib().vcg_randn(_ptr(out), out.numel(), int(seed), int(offset), _stream()), "vcg_randn")
    return out


def rand_uniform(shape, device, seed, offset=0):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _native.check(_native.lib().vcg_rand_uniform(_ptr(out), out.numel(), int(seed), int(offset), _stream()), "vcg_rand_uniform")
    return out


def adam_step_flat(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale=1.0):
    """One fused launch of torch's single-tensor Adam formula over flat buffers."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    step_size = lr / bc1
    bc2_sqrt = math.sqrt(bc2)
    _native.check(_native.lib().vcg_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), step_size, beta1, beta2,
                                              1.0 - beta1, 1.0 - beta2, eps, bc2_sqrt, grad_scale, _stream()), "vcg_adam_step")
    PARAM_EPOCH[0] += 1


def grad_norm_workspace(n, device):
    """The slot buffer vcg_grad_norm needs for n gradients (its own allocation: it lives as long as the optimizer)."""
    return torch.empty(_native.lib().vcg_grad_norm_workspace(int(n)) // 4, dtype=torch.float32, device=device)


def grad_norm(flat_grad, grad_scale, max_norm, out, ws):
    """out[0:4] = [grad_scale * ||flat_grad||_2, min(1, max_norm / (norm + 1e-6)), 1.0 if a gradient is NaN / Inf else 0.0, 0]
    on the device: one deterministic reduction in double (csrc/grad_clip.hip), nothing comes back to the host."""
    _require_gpu(flat_grad, "grad_norm")
    _require_gpu(out, "grad_norm")
    if not flat_grad.is_contiguous() or out.numel() < 4:
        raise RuntimeError("grad_norm: flat_grad must be contiguous and out hold four floats")
    _native.check(_native.lib().vcg_grad_norm(_ptr(flat_grad), flat_grad.numel(), float(grad_scale), float(max_norm), _ptr(out),
                                              _ptr(ws), ws.numel() * 4, _stream()), "vcg_grad_norm")
    return out


def adam_step_flat_clipped(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale, clip):
    """adam_step_flat with the gradient scaled by clip[1] on the device, or no update at all where clip[2] != 0
    (`clip`: what grad_norm wrote)."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    step_size = lr / bc1
    bc2_sqrt = math.sqrt(bc2)
    _native.check(_native.lib().vcg_adam_step_clipped(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), step_size, beta1, beta2,
                                                      1.0 - beta1, 1.0 - beta2, eps, bc2_sqrt, grad_scale, _ptr(clip), _stream()),
                  "vcg_adam_step_clipped")
    PARAM_EPOCH[0] += 1


def ema_update(ema, param, weight, skip=None):
    """ema += weight * (param - ema) in place, one launch (csrc/ema.hip); `weight` = 1 - decay as a Python float (double), rounded
    to fp32 once on the way in.  weight 1 copies, weight 0 launches nothing.  `skip`: FusedAdam.clip_state or None: a step Adam
    skipped for a NaN / Inf gradient leaves the average alone too."""
    _require_gpu(ema, "ema_update")
    _require_gpu(param, "ema_update")
    if not ema.is_contiguous() or not param.is_contiguous() or ema.numel() != param.numel():
        raise RuntimeError("ema_update: ema and param must be contiguous and of one size")
    if skip is not None:
        _require_gpu(skip, "ema_update")
        if not skip.is_contiguous() or skip.numel() < 4:
            raise RuntimeError("ema_update: skip must hold the four floats grad_norm wrote")
    _native.check(_native.lib().vcg_ema_update(_ptr(ema), _ptr(param), ema.numel(), float(weight), _ptr(skip), _stream()),
                  "vcg_ema_update")
    return ema


def swap_(a, b):
    """Exchange the contents of two flat buffers in place, one launch (csrc/ema.hip).  The caller orders it against other
    streams and bumps the parameter epochs if one of the two holds parameters (FusedAdam.swap_ema)."""
    _require_gpu(a, "swap_")
    _require_gpu(b, "swap_")
    if not a.is_contiguous() or not b.is_contiguous() or a.numel() != b.numel():
        raise RuntimeError("swap_: the two tensors must be contiguous and of one size")
    _native.check(_native.lib().vcg_swap(_ptr(a), _ptr(b), a.numel(), _stream()), "vcg_swap")


# ------------------------------------------------------------------ evaluation (test.py)
def _images_phys(t, what):
    """A logical (N, 3, S, S) image batch -> its (N, S, S, 4) physical buffer (alias or converted copy)."""
    if t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != t.shape[3]:
        raise RuntimeError(f"{what}: expected an (N, 3, S, S) image batch, got shape {tuple(t.shape)}")
    return as_phys(t)


def image_metrics(out, target):
    """Per-image [l1, mse, psnr, ssim] of clamp(out, 0, 1) against `target`, both logical (N, 3, S, S) with S >= 11 ->
    an (N, 4) fp32 device tensor (psnr is +inf where mse == 0).  csrc/metrics.hip has the definitions."""
    _require_gpu(out, "image_metrics")
    _require_gpu(target, "image_metrics")
    if out.shape != target.shape:
        raise RuntimeError(f"image_metrics: shape mismatch {tuple(out.shape)} vs {tuple(target.shape)}")
    op, tp = _images_phys(out, "image_metrics"), _images_phys(target, "image_metrics")
    n, s = out.shape[0], out.shape[2]
    if s < 11:
        raise RuntimeError(f"image_metrics: SSIM's 11x11 window needs images of at least 11x11, got {s}x{s}")
    tiles = (s + 15) // 16
    ws = torch.empty(n * tiles * tiles * 4, dtype=torch.float32, device=out.device)
    res = torch.empty((n, 4), dtype=torch.float32, device=out.device)
    _native.check(_native.lib().vcg_image_metrics(_ptr(op), _ptr(tp), _ptr(res), n, s, _ptr(ws), ws.numel() * 4, _stream()),
                  "vcg_image_metrics")
    return res


def to_display(x, uint8=False):
    """Logical (N, 3, S, S) images -> contiguous (N, S, S, 3) on the device: fp32 clamped to [0, 1], or uint8
    floor(255 v + 0.5) clipped to 0..255 (PNG pixels)."""
    _require_gpu(x, "to_display")
    xp = _images_phys(x, "to_display")
    n, s = x.shape[0], x.shape[2]
    dst = torch.empty((n, s, s, 3), dtype=torch.uint8 if uint8 else torch.float32, device=x.device)
    _native.check(_native.lib().vcg_to_display(_ptr(xp), _ptr(dst), n, s, 1 if uint8 else 0, _stream()), "vcg_to_display")
    return dst


# ------------------------------------------------------------------ whole images of any size (translate.py)
# The largest N * Hp * Wp (padded pixels of one batch) a generator forward accepts.  Every kernel a forward dispatches to computes
# element offsets in size_t except the gathers of the direct convolution kernels (conv_igemm.hip, conv_slab.hip), which address
# their input with 32-bit BYTE offsets and keep 0x80000000 as the "outside" mark; vcg_conv_fwd* therefore refuse an input of
# 2 GiB or more.  The largest input of a generator is a 64-channel full-resolution map (the first D block's and the head's):
# N * Hp * Wp * 64 * 4 bytes < 2^31.  DESIGN.md, "The translator".
MAX_TRANSLATE_PIXELS = (1 << 31) // (64 * 4) - 1
MIN_TRANSLATE_SIDE = 32           # the 1/16-resolution bottleneck is reflect-padded by 1: it must be at least 2 x 2


def pad_plan(h, w):
    """(Hp, Wp, top, left): H and W rounded up to multiples of 16 (four PixelUnshuffles), the frame centred in the padded one."""
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    return hp, wp, (hp - h) // 2, (wp - w) // 2


def reflect_index(n, before, total):
    """Source index of each of `total` padded positions of an axis of n samples that starts `before` positions early:
    reflection without repeating the edge sample (numpy.pad(mode="reflect"), the convolutions' own padding)."""
    i = [abs(k - before) for k in range(total)]
    return [2 * (n - 1) - k if k >= n else k for k in i]


def check_translate_size(n, h, w):
    """Raise before anything is launched if a batch of n frames of h x w cannot go through a generator in one piece."""
    if h < MIN_TRANSLATE_SIDE or w < MIN_TRANSLATE_SIDE:
        raise RuntimeError(f"a {h}x{w} frame is smaller than {MIN_TRANSLATE_SIDE} on a side: after four halvings the bottleneck map "
                           f"would be too small for its reflection padding")
    hp, wp, _, _ = pad_plan(h, w)
    if n * hp * wp > MAX_TRANSLATE_PIXELS:
        raise RuntimeError(f"{n} frame(s) of {h}x{w} ({n * hp * wp} padded pixels) exceed ops.MAX_TRANSLATE_PIXELS = "
                           f"{MAX_TRANSLATE_PIXELS}: the convolution kernels address a tensor with 32-bit byte offsets.  There is no "
                           f"tiled fallback: InstanceNorm statistics are taken over the whole image, so tiles would not reproduce "
                           f"the whole-frame result.  Use a smaller batch or a smaller frame")
    return hp, wp


def image_load(frames):
    """uint8 device frames (N, H, W, C), C in (1, 3, 4) -> (logical (N, 3, Hp, Wp) nhwc batch in [0, 1], (top, left, H, W)): v / 255,
    grey replicated, alpha dropped, padded by reflection to multiples of 16 with the frame centred (csrc/image_io.hip)."""
    if not frames.is_cuda:
        raise RuntimeError(f"image_load: expected a tensor on the MI355X (cuda) device, got {frames.device}; this package has no CPU path")
    if frames.dim() != 4 or frames.dtype != torch.uint8 or frames.shape[3] not in (1, 3, 4):
        raise RuntimeError(f"image_load: expected uint8 (N, H, W, C) frames with C in (1, 3, 4), got {frames.dtype} {tuple(frames.shape)}")
    src = frames.contiguous()
    n, h, w, c = src.shape
    hp, wp, top, left = pad_plan(h, w)
    dst = torch.empty((n, hp, wp, 4), dtype=torch.float32, device=src.device)
    _native.check(_native.lib().vcg_image_load(_ptr(src), _ptr(dst), n, h, w, c, hp, wp, top, left, _stream()), "vcg_image_load")
    return logical_of(dst, 3), (top, left, h, w)


def _window_of(t, window, what):
    if t.dim() != 4 or t.shape[1] != 3:
        raise RuntimeError(f"{what}: expected an (N, 3, H, W) image batch, got shape {tuple(t.shape)}")
    n, _, hp, wp = t.shape
    top, left, h, w = (0, 0, hp, wp) if window is None else window
    if top < 0 or left < 0 or h < 1 or w < 1 or top + h > hp or left + w > wp:
        raise RuntimeError(f"{what}: the window {tuple(window)} leaves the {hp}x{wp} images")
    return n, hp, wp, top, left, h, w


def to_display_hw(x, window=None, uint8=False):
    """`to_display` for images of any height and width, cropped to `window` = (top, left, H, W) (None: the whole image)."""
    _require_gpu(x, "to_display_hw")
    n, hp, wp, top, left, h, w = _window_of(x, window, "to_display_hw")
    xp = as_phys(x)
    dst = torch.empty((n, h, w, 3), dtype=torch.uint8 if uint8 else torch.float32, device=x.device)
    _native.check(_native.lib().vcg_to_display_hw(_ptr(xp), _ptr(dst), n, hp, wp, top, left, h, w, 1 if uint8 else 0, _stream()),
                  "vcg_to_display_hw")
    return dst


def image_metrics_hw(out, target, window=None):
    """`image_metrics` over `window` = (top, left, H, W) of two (N, 3, Hp, Wp) batches, H, W >= 11 (None: the whole images).
    Nothing outside the window is read; for whole square images the result is `image_metrics`'s, bit for bit."""
    _require_gpu(out, "image_metrics_hw")
    _require_gpu(target, "image_metrics_hw")
    if out.shape != target.shape:
        raise RuntimeError(f"image_metrics_hw: shape mismatch {tuple(out.shape)} vs {tuple(target.shape)}")
    n, hp, wp, top, left, h, w = _window_of(out, window, "image_metrics_hw")
    if h < 11 or w < 11:
        raise RuntimeError(f"image_metrics_hw: SSIM's 11x11 window needs images of at least 11x11, got {h}x{w}")
    op, tp = as_phys(out), as_phys(target)
    ws = torch.empty(n * ((h + 15) // 16) * ((w + 15) // 16) * 4, dtype=torch.float32, device=out.device)
    res = torch.empty((n, 4), dtype=torch.float32, device=out.device)
    _native.check(_native.lib().vcg_image_metrics_hw(_ptr(op), _ptr(tp), _ptr(res), n, hp, wp, top, left, h, w, _ptr(ws),
                                                     ws.numel() * 4, _stream()), "vcg_image_metrics_hw")
    return res


# ------------------------------------------------------------------ the sampling translator (translate.py --samples K)
def _latent_phys(mu, logvar, what):
    _require_gpu(mu, what)
    _require_gpu(logvar, what)
    if mu.dim() != 4 or mu.shape != logvar.shape:
        raise RuntimeError(f"{what}: mu and logvar must be two (N, C, h, w) maps of one shape, got {tuple(mu.shape)} and {tuple(logvar.shape)}")
    return as_phys(mu), as_phys(logvar)


def reserve_eps_many(mu, samples):
    """Reserve the eps draws of `samples` reparameterisations of every map of `mu` (logical (N, C, h, w)): the stream advances
    once, by N * samples * per / 4 counters (per: floats of one physical map), and the position is returned for
    `reparameterize_many(seed_offset=)`, whose chunks then draw inside the reservation."""
    n, c, h, w = mu.shape
    off = _RNG["offset"]
    _RNG["offset"] += n * int(samples) * (h * w * pitch(c) // 4)
    return off


def reparameterize_many(mu, logvar, samples, first=0, count=None, eps=None, temperature=1.0, seed_offset=None):
    """Inference only (no autograd node): the samples first .. first + count - 1 of the `samples` of every latent map,
    z[(n, j)] = mu[n] + temperature * eps[(n, j)] * exp(0.5 * clamp(logvar[n], -10, 10)) -> (z, eps used), logical
    (N * count, C, h, w) batches with sample j of map n at index n * count + (j - first): what a decoder takes.
    eps: None draws on the device — sample (n, j) at `seed_offset` + (n * samples + j) * per / 4 of the ops stream, whatever the
    chunking; `seed_offset` None reserves the whole batch here (reserve_eps_many) and is only allowed for a call that covers all
    the samples.  eps given: the chunk's noise, logical (N, count, C, h, w) (parity runs); the stream does not move."""
    mup, lvp = _latent_phys(mu, logvar, "reparameterize_many")
    n, c, h, w = mu.shape
    samples, first = int(samples), int(first)
    count = samples - first if count is None else int(count)
    per = h * w * pitch(c)
    z = torch.empty((n * max(count, 0), h, w, pitch(c)), dtype=torch.float32, device=mu.device)
    used = torch.empty_like(z)
    epsp, off = None, 0
    if eps is not None:
        if tuple(eps.shape) != (n, count, c, h, w):
            raise RuntimeError(f"reparameterize_many: eps has shape {tuple(eps.shape)}, expected {(n, count, c, h, w)}")
        epsp = as_phys(eps.to(mu.device).reshape(n * count, c, h, w))
    elif seed_offset is None:
        if first != 0 or count != samples:
            raise RuntimeError("reparameterize_many: a chunk of a batch needs the batch's seed_offset (ops.reserve_eps_many): the "
                               "eps stream advances once per batch, not per chunk")
        off = reserve_eps_many(mu, samples)
    else:
        off = int(seed_offset)
    _native.check(_native.lib().vcg_reparam_many_fwd(_ptr(mup), _ptr(lvp), _ptr(epsp), _ptr(used), _ptr(z), n, samples, first, count, per,
                                                     float(temperature), _RNG["seed"], off, _stream()), "vcg_reparam_many_fwd")
    return logical_of(z, c), logical_of(used, c)


def sample_accumulate(y, mean, m2, samples_in_chunk, seen):
    """Fold a chunk of decoded samples into running statistics, in place (csrc/sample_stats.hip): y logical
    (N * samples_in_chunk, 3, Hp, Wp) with sample j of frame n at index n * samples_in_chunk + j; mean, m2 logical (N, 3, Hp, Wp) nhwc
    views (`logical_of(torch.empty((N, Hp, Wp, 4)), 3)`): Welford's mean and sum of squared deviations of clamp(y, 0, 1) after
    `seen` + samples_in_chunk samples.  seen == 0 initialises them (they need not be cleared)."""
    _require_gpu(y, "sample_accumulate")
    k = int(samples_in_chunk)
    for t, name in ((mean, "mean"), (m2, "m2")):
        _require_gpu(t, "sample_accumulate")
        if t.dim() != 4 or t.shape[1] != 3 or not can_alias(t):
            raise RuntimeError(f"sample_accumulate: {name} must be a logical (N, 3, Hp, Wp) nhwc view, got shape {tuple(t.shape)}")
    n, _, hp, wp = mean.shape
    if mean.shape != m2.shape or k < 1 or tuple(y.shape) != (n * k, 3, hp, wp):
        raise RuntimeError(f"sample_accumulate: y {tuple(y.shape)} is not {k} sample(s) of each of the {n} frames of mean "
                           f"{tuple(mean.shape)} / m2 {tuple(m2.shape)}")
    _native.check(_native.lib().vcg_sample_accumulate(_ptr(as_phys(y)), _ptr(phys_of(mean)), _ptr(phys_of(m2)), n, k, int(seen),
                                                      hp * wp, _stream()), "vcg_sample_accumulate")
    return mean, m2


def spread_display_hw(m2, count, window=None, gain=2.0, uint8=False):
    """The spread map of `count` >= 2 folded samples over `window` = (top, left, H, W) of m2 (logical (N, 3, Hp, Wp); None: the
    whole image): per pixel the RMS over the channels of the unbiased sample standard deviation -> (map, per-image mean of the
    map as (N,) fp32).  map: (N, H, W) fp32, with `uint8` the grey image floor(255 min(1, gain s) + 0.5), with uint8="both" the
    pair (fp32, uint8) from the one launch."""
    _require_gpu(m2, "spread_display_hw")
    n, hp, wp, top, left, h, w = _window_of(m2, window, "spread_display_hw")
    lib = _native.lib()
    ws = torch.empty(max(lib.vcg_spread_workspace(n, h, w), 16) // 4, dtype=torch.float32, device=m2.device)
    f32 = torch.empty((n, h, w), dtype=torch.float32, device=m2.device) if uint8 in (False, "both") else None
    u8 = torch.empty((n, h, w), dtype=torch.uint8, device=m2.device) if uint8 in (True, "both") else None
    res = torch.empty((n,), dtype=torch.float32, device=m2.device)
    _native.check(lib.vcg_spread_display_hw(_ptr(as_phys(m2)), int(count), float(gain), _ptr(f32), _ptr(u8), _ptr(res), n, hp, wp, top,
                                            left, h, w, _ptr(ws), ws.numel() * 4, _stream()), "vcg_spread_display_hw")
    return ((f32, u8) if uint8 == "both" else u8 if uint8 else f32), res


# ------------------------------------------------------------------ the interpolating translator (translate.py --interpolate N)
LATENT_PATH_MODES = ("slerp", "lerp")                # the index is the library's VCG_LATENT_* code


def _pair_phys_maps(a, b, what):
    _require_gpu(a, what)
    _require_gpu(b, what)
    if a.dim() != 4 or a.shape != b.shape or a.shape[0] < 1:
        raise RuntimeError(f"{what}: a and b must be two (P, C, h, w) maps of one shape with P >= 1, got {tuple(a.shape)} and {tuple(b.shape)}")
    return as_phys(a), as_phys(b)                    # two views of one encoder batch (mu[:-1], mu[1:]) alias it: nothing is copied


def latent_pair_stats(a, b):
    """[sum a[p]^2, sum b[p]^2, sum a[p] b[p]] of each pair of logical (P, C, h, w) latent maps, over the logical channels, summed
    in double in a fixed order -> a device (P, 3) float64 tensor (csrc/latent_path.hip).  Inference only."""
    ap, bp = _pair_phys_maps(a, b, "latent_pair_stats")
    n, c, h, w = a.shape
    per = h * w * pitch(c)
    lib = _native.lib()
    ws = torch.empty(max(lib.vcg_latent_stats_workspace(n, per), 8) // 8, dtype=torch.float64, device=a.device)
    out = torch.empty((n, 3), dtype=torch.float64, device=a.device)
    _native.check(lib.vcg_latent_pair_stats(_ptr(ap), _ptr(bp), _ptr(out), n, per, c, pitch(c), _ptr(ws), ws.numel() * 8, _stream()),
                  "vcg_latent_pair_stats")
    return out


def latent_path(a, b, steps, mode="slerp", first=0, count=None, stats=None, return_coef=False):
    """Inference only (no autograd node): the fractions first .. first + count - 1 of the T = steps + 2 uniform fractions
    t_j = j / (T - 1) of the path from a[p] to b[p], logical (P, C, h, w) maps -> a logical (P * count, C, h, w) batch with fraction
    j of pair p at index p * count + (j - first): what a decoder takes.  `steps` counts the INTERMEDIATE frames; j == 0 is a[p] and
    j == T - 1 is b[p], bit for bit.  mode "slerp": z = (sin((1 - t) w) a + sin(t w) b) / sin(w) with w the angle between the two
    maps, the straight line where they are (anti)parallel or empty (VCG_SLERP_MIN_SIN); "lerp": z = (1 - t) a + t b.  A value does
    not depend on the chunking (first, count).  stats: `latent_pair_stats(a, b)` if the caller has it (the slerp computes it
    otherwise; the lerp does not use it).  return_coef: also the (P, count, 2) fp32 coefficients (ca, cb) that were used."""
    if mode not in LATENT_PATH_MODES:
        raise ValueError(f"latent_path: mode must be one of {LATENT_PATH_MODES}, got {mode!r}")
    ap, bp = _pair_phys_maps(a, b, "latent_path")
    n, c, h, w = a.shape
    total = int(steps) + 2
    first = int(first)
    count = total - first if count is None else int(count)
    if total < 2 or count < 1 or first < 0 or first + count > total:
        raise RuntimeError(f"latent_path: steps={steps}, first={first}, count={count}: the path has the {max(total, 0)} fractions "
                           f"0 .. steps + 1 and a call takes at least one of them")
    if mode == "slerp":
        if stats is None:
            stats = latent_pair_stats(a, b)
        elif not stats.is_cuda or stats.dtype != torch.float64 or tuple(stats.shape) != (n, 3) or not stats.is_contiguous():
            raise RuntimeError(f"latent_path: stats must be latent_pair_stats's (P, 3) float64 device tensor, got {stats.dtype} "
                               f"{tuple(stats.shape)} on {stats.device}")
    else:
        stats = None
    z = torch.empty((n * count, h, w, pitch(c)), dtype=torch.float32, device=a.device)
    coef = torch.empty((n, count, 2), dtype=torch.float32, device=a.device) if return_coef else None
    _native.check(_native.lib().vcg_latent_path(_ptr(ap), _ptr(bp), _ptr(stats), _ptr(z), _ptr(coef), n, total, first, count,
                                                h * w * pitch(c), c, pitch(c), LATENT_PATH_MODES.index(mode), _stream()), "vcg_latent_path")
    return (logical_of(z, c), coef) if return_coef else logical_of(z, c)


# ------------------------------------------------------------------ sliced Wasserstein distance (swd.py, csrc/swd.hip)
SWD_MAX_DESC = 16384              # descriptors per set and level: a sorted column lives in 64 KiB of LDS (VCG_SWD_MAX_DESC)
SWD_PATCH = 7
SWD_DESC = 3 * SWD_PATCH * SWD_PATCH
SWD_MIN_SIDE = 16                 # the coarsest pyramid level


def swd_level_sizes(s):
    """Sides of the Laplacian-pyramid levels of an S x S image: every S / 2^k that is whole and at least 16."""
    s = int(s)
    if s < SWD_MIN_SIDE:
        raise RuntimeError(f"sliced Wasserstein distance: images of {s}x{s} are smaller than the coarsest pyramid level "
                           f"({SWD_MIN_SIDE}x{SWD_MIN_SIDE})")
    sizes = [s]
    while sizes[-1] % 2 == 0 and sizes[-1] // 2 >= SWD_MIN_SIDE:
        sizes.append(sizes[-1] // 2)
    return sizes


def laplacian_pyramid(images):
    """Logical (N, 3, S, S) images, S >= 16 -> [L_0 .. L_{L-1}], logical (N, 3, S_k, S_k) nhwc views: the Laplacian pyramid of
    clamp(images, 0, 1) with the 5-tap binomial kernel and mirrored borders, one launch per level; the last level is the
    Gaussian residual."""
    _require_gpu(images, "laplacian_pyramid")
    g = _images_phys(images, "laplacian_pyramid")
    n, s = images.shape[0], images.shape[2]
    sizes = swd_level_sizes(s)
    lib, out = _native.lib(), []
    for k, sk in enumerate(sizes):
        last = k == len(sizes) - 1
        if last and k > 0:
            out.append(g)                            # the residual is the previous launch's G
            break
        lap = torch.empty((n, sk, sk, 4), dtype=torch.float32, device=images.device)
        nxt = None if last else torch.empty((n, sk // 2, sk // 2, 4), dtype=torch.float32, device=images.device)
        _native.check(lib.vcg_swd_pyramid_level(_ptr(g), _ptr(nxt), _ptr(lap), n, sk, 1 if k == 0 else 0, _stream()),
                      "vcg_swd_pyramid_level")
        out.append(lap)
        g = nxt
    return [logical_of(t, 3) for t in out]


def swd_gather(level, plan, out=None, row_offset=0):
    """The 7x7x3 patches of `level` (logical (N, 3, S, S)) named by `plan`, an int32 host array of (image, top, left) rows, as
    rows row_offset .. of the (rows, 147) fp32 descriptor matrix `out` (None: a fresh matrix of len(plan) rows).  A patch is
    flattened as (c, dy, dx).  The plan is read on the host and passed to the kernel by value."""
    import numpy as np
    _require_gpu(level, "swd_gather")
    lp = _images_phys(level, "swd_gather")
    plan = np.ascontiguousarray(plan, dtype=np.int32)
    if plan.ndim != 2 or plan.shape[1] != 3:
        raise RuntimeError(f"swd_gather: the plan must be (count, 3) rows of (image, top, left), got shape {plan.shape}")
    count = plan.shape[0]
    if out is None:
        out = torch.empty((count, SWD_DESC), dtype=torch.float32, device=level.device)
    _require_gpu(out, "swd_gather")
    if out.dim() != 2 or out.shape[1] != SWD_DESC or not out.is_contiguous():
        raise RuntimeError(f"swd_gather: out must be a contiguous (rows, {SWD_DESC}) matrix, got shape {tuple(out.shape)}")
    _native.check(_native.lib().vcg_swd_gather(_ptr(lp), level.shape[0], level.shape[2], plan.ctypes.data_as(_native._I32P), count,
                                               _ptr(out), int(row_offset), out.shape[0], _stream()), "vcg_swd_gather")
    return out


def _swd_desc(desc, what):
    _require_gpu(desc, what)
    if desc.dim() != 2 or not desc.is_contiguous():
        raise RuntimeError(f"{what}: expected a contiguous (n, k) matrix, got shape {tuple(desc.shape)}")
    if not 1 <= desc.shape[0] <= SWD_MAX_DESC:
        raise RuntimeError(f"{what}: {desc.shape[0]} descriptors (1 .. {SWD_MAX_DESC})")


def swd_normalize(desc):
    """(n, 147) descriptors -> (desc - mean_c) / std_c per channel c (columns 49 c .. 49 c + 48): mean and population standard
    deviation over all rows and the channel's patch pixels, deterministic (a constant channel comes out NaN)."""
    _swd_desc(desc, "swd_normalize")
    if desc.shape[1] != SWD_DESC:
        raise RuntimeError(f"swd_normalize: expected {SWD_DESC} columns, got {desc.shape[1]}")
    n = desc.shape[0]
    ws = torch.empty(_scratch("vcg_swd_normalize_workspace", n) // 4, dtype=torch.float32, device=desc.device)
    out = torch.empty_like(desc)
    _call("vcg_swd_normalize", _ptr(desc), _ptr(out), n, _ptr(ws), ws.numel() * 4, _stream())
    return out


def swd_project(desc, directions):
    """desc (n, k) x directions (k, d) -> the (n, d) projections, fp32 products and sums on the fp32 MFMA.  The result is stored
    transposed (strides (1, n)): each direction's projections are contiguous, which is what `sort_columns` reads fastest."""
    _swd_desc(desc, "swd_project")
    _require_gpu(directions, "swd_project")
    if directions.dim() != 2 or not directions.is_contiguous() or directions.shape[0] != desc.shape[1]:
        raise RuntimeError(f"swd_project: directions must be a contiguous ({desc.shape[1]}, d) matrix, got shape "
                           f"{tuple(directions.shape)}")
    n, k, d = desc.shape[0], desc.shape[1], directions.shape[1]
    out = torch.empty((d, n), dtype=torch.float32, device=desc.device)
    _call("vcg_swd_project", _ptr(desc), _ptr(directions), _ptr(out), n, k, d, _stream())
    return out.t()


def sort_columns(x):
    """Every column of an (n, cols) fp32 matrix sorted ascending over the rows, n <= 16384: a bitonic network in LDS, one
    workgroup per column.  x is row-major or the transposed view `swd_project` returns; the result has x's layout."""
    _require_gpu(x, "sort_columns")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise RuntimeError(f"sort_columns: expected an (n, cols) matrix, got shape {tuple(x.shape)}")
    n, cols = x.shape
    if n > SWD_MAX_DESC:
        raise RuntimeError(f"sort_columns: {n} rows exceed {SWD_MAX_DESC}: a column is sorted in 64 KiB of LDS")
    if x.is_contiguous():
        rs, cs = cols, 1
    elif x.t().is_contiguous():
        rs, cs = 1, n
    else:
        raise RuntimeError("sort_columns: the matrix must be contiguous or the transpose of a contiguous one")
    out = torch.empty_like(x.t()).t() if rs == 1 else torch.empty_like(x)
    _call("vcg_sort_columns", _ptr(x), _ptr(out), n, cols, rs, cs, _stream())
    return out


def swd_distance(a, b):
    """mean |a - b| of two equally laid out matrices, summed in double in a fixed order -> a 0-d fp32 device tensor."""
    _require_gpu(a, "swd_distance")
    _require_gpu(b, "swd_distance")
    if a.shape != b.shape or a.stride() != b.stride() or a.numel() == 0:
        raise RuntimeError(f"swd_distance: shape / layout mismatch {tuple(a.shape)} {a.stride()} vs {tuple(b.shape)} {b.stride()}")
    if not (a.is_contiguous() or (a.dim() == 2 and a.t().is_contiguous())):
        raise RuntimeError("swd_distance: the matrices must be dense")
    n = a.numel()
    ws = torch.empty(_scratch("vcg_swd_distance_workspace", n) // 4, dtype=torch.float32, device=a.device)
    out = torch.empty((), dtype=torch.float32, device=a.device)
    _call("vcg_swd_distance", _ptr(a), _ptr(b), _ptr(out), n, _ptr(ws), ws.numel() * 4, _stream())
    return out


# ------------------------------------------------------------------ sliced Wasserstein training loss (csrc/swd_loss.hip)
SWD_LOSS_MAX_DESC = 8192          # descriptors per set and level: keys and source rows of a column, 64 KiB of LDS (VCG_SWD_LOSS_MAX_DESC)
SWD_LOSS_MAX_LEVELS = 3
SWD_LOSS_DIRS = 128               # directions per step


class SwdPlan(NamedTuple):
    """What one evaluation of `swd_loss` draws: the in-cell patch offset (oy, ox) of every level, and the (147, 128) matrix of
    unit directions on the device (Losses.SlicedWassersteinLoss draws both)."""
    offsets: tuple
    directions: torch.Tensor


def _swd_int(value, name, what):
    if isinstance(value, bool) or not hasattr(value, "__index__"):
        raise RuntimeError(f"{what}: {name} must be an integer, got {value!r}")
    return int(value)


def swd_loss_levels(h, w):
    """How many levels (at most 3) the loss has on H x W images: level k + 1 is the 2 x 2 mean of level k and exists while both
    sides of level k are even and their halves at least 16."""
    levels = _native.lib().vcg_swd_loss_levels(_swd_int(h, "h", "swd_loss_levels"), _swd_int(w, "w", "swd_loss_levels"))
    if levels == 0:
        _native.check(-1, "vcg_swd_loss_levels")
    return levels


def swd_cell_side(n_images, h, w):
    """The side s of the cells a level of `n_images` H x W maps is cut into: the smallest s >= 8 that leaves at most 8192 cells
    (one descriptor each) in the set."""
    s = _native.lib().vcg_swd_cell_side(*(_swd_int(v, k, "swd_cell_side") for k, v in (("n_images", n_images), ("h", h), ("w", w))))
    if s == 0:
        _native.check(-1, "vcg_swd_cell_side")
    return s


def _swd_phys(t, what):
    _require_gpu(t, what)
    if t.dim() != 4 or t.shape[3] != 4 or not t.is_contiguous():
        raise RuntimeError(f"{what}: expected a contiguous physical (N, H, W, 4) image tensor, got shape {tuple(t.shape)}")
    return t.shape[0], t.shape[1], t.shape[2]


def swd_pool(x):
    """Physical (N, H, W, 4) -> (N, H/2, W/2, 4): the 2 x 2 mean, rounded once; channel 3 is 0."""
    n, h, w = _swd_phys(x, "swd_pool")
    out = torch.empty((n, h // 2, w // 2, 4), dtype=torch.float32, device=x.device)
    _call("vcg_swd_pool", _ptr(x), _ptr(out), n, h, w, _stream())
    return out


def swd_pool_adjoint_add(coarse, fine):
    """fine (N, H, W, 4) += coarse (N, H/2, W/2, 4) / 4, in place: the adjoint of `swd_pool` added into the finer gradient map."""
    n, h, w = _swd_phys(fine, "swd_pool_adjoint_add")
    nc, hc, wc = _swd_phys(coarse, "swd_pool_adjoint_add")
    if (n, h, w) != (nc, 2 * hc, 2 * wc):
        raise RuntimeError(f"swd_pool_adjoint_add: coarse {tuple(coarse.shape)} is not the half-size map of fine {tuple(fine.shape)}")
    _call("vcg_swd_pool_adjoint_add", _ptr(coarse), _ptr(fine), n, h, w, _stream())
    return fine


def swd_grid_gather(level, s, oy, ox):
    """The 7x7x3 patch at in-cell offset (oy, ox) of every s x s cell of the physical (N, H, W, 4) `level` -> (n, 147), row
    (image, cell row, cell column), a patch flattened as (c, dy, dx)."""
    n, h, w = _swd_phys(level, "swd_grid_gather")
    s, oy, ox = (_swd_int(v, k, "swd_grid_gather") for k, v in (("s", s), ("oy", oy), ("ox", ox)))
    rows = n * (h // s) * (w // s) if s > 0 else 0
    out = torch.empty((max(rows, 1), SWD_DESC), dtype=torch.float32, device=level.device)
    _call("vcg_swd_grid_gather", _ptr(level), _ptr(out), n, h, w, s, oy, ox, _stream())
    return out


def swd_grid_scatter(gdesc, shape, s, oy, ox, scale=1.0, g=None):
    """The adjoint of `swd_grid_gather` on a level of `shape` = (N, H, W): a fresh physical (N, H, W, 4) map holding every element
    of gdesc (n, 147), times `scale` and the device scalar `g` if given, at its pixel, and +0 everywhere else."""
    _require_gpu(gdesc, "swd_grid_scatter")
    n, h, w = (_swd_int(v, "shape", "swd_grid_scatter") for v in shape)
    s, oy, ox = (_swd_int(v, k, "swd_grid_scatter") for k, v in (("s", s), ("oy", oy), ("ox", ox)))
    rows = n * (h // s) * (w // s) if s > 0 else 0
    if gdesc.dim() != 2 or not gdesc.is_contiguous() or (rows > 0 and tuple(gdesc.shape) != (rows, SWD_DESC)):
        raise RuntimeError(f"swd_grid_scatter: gdesc must be a contiguous ({rows}, {SWD_DESC}) matrix, got shape {tuple(gdesc.shape)}")
    if g is not None:
        _require_gpu(g, "swd_grid_scatter")
        if g.numel() != 1:
            raise RuntimeError(f"swd_grid_scatter: g must hold one value, got shape {tuple(g.shape)}")
    out = torch.empty((max(n, 1), max(h, 1), max(w, 1), 4), dtype=torch.float32, device=gdesc.device)
    _call("vcg_swd_grid_scatter", _ptr(gdesc), _ptr(g), float(scale), _ptr(out), n, h, w, s, oy, ox, _stream())
    return out


def sort_columns_indexed(x):
    """`sort_columns` that remembers where each key came from: (keys, rows), both with x's layout, rows int32; ordered by
    (key, row), which is what a stable argsort gives.  n <= 8192."""
    _require_gpu(x, "sort_columns_indexed")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise RuntimeError(f"sort_columns_indexed: expected an (n, cols) matrix, got shape {tuple(x.shape)}")
    n, cols = x.shape
    if n > SWD_LOSS_MAX_DESC:
        raise RuntimeError(f"sort_columns_indexed: {n} rows exceed {SWD_LOSS_MAX_DESC}: a column's keys and rows are sorted in 64 KiB of LDS")
    if x.is_contiguous():
        rs, cs = cols, 1
    elif x.t().is_contiguous():
        rs, cs = 1, n
    else:
        raise RuntimeError("sort_columns_indexed: the matrix must be contiguous or the transpose of a contiguous one")
    keys = torch.empty_like(x.t()).t() if rs == 1 else torch.empty_like(x)
    rows = torch.empty(keys.t().shape if rs == 1 else keys.shape, dtype=torch.int32, device=x.device)
    rows = rows.t() if rs == 1 else rows
    _call("vcg_sort_columns_indexed", _ptr(x), _ptr(keys), _ptr(rows), n, cols, rs, cs, _stream())
    return keys, rows


def swd_pair_loss(a_sorted, b_sorted, perm_a, weight=1.0, total=None):
    """One level's value and signed gradient from the sorted projections, (n, D) views with strides (1, n) as `swd_project`
    and the sorts hand them over: -> (out, gproj, total).  total (one float64 on the device; None: a fresh one, started at 0)
    += weight * mean |a_sorted - b_sorted|, out = float32(total) as a 0-dim tensor, gproj (D, n) contiguous with
    gproj[d][perm_a[i][d]] = sign(a_sorted[i][d] - b_sorted[i][d]), not scaled."""
    _require_gpu(a_sorted, "swd_pair_loss")
    _require_gpu(b_sorted, "swd_pair_loss")
    if a_sorted.dim() != 2 or a_sorted.numel() == 0 or not a_sorted.t().is_contiguous():
        raise RuntimeError(f"swd_pair_loss: expected (n, D) projections with strides (1, n), got shape {tuple(a_sorted.shape)} "
                           f"strides {a_sorted.stride()}")
    for t, name in ((b_sorted, "b_sorted"), (perm_a, "perm_a")):
        if t.shape != a_sorted.shape or t.stride() != a_sorted.stride() or t.device != a_sorted.device:
            raise RuntimeError(f"swd_pair_loss: {name} {tuple(t.shape)} {t.stride()} does not match a_sorted {tuple(a_sorted.shape)} "
                               f"{a_sorted.stride()}")
    if perm_a.dtype != torch.int32:
        raise RuntimeError(f"swd_pair_loss: perm_a must be int32, got {perm_a.dtype}")
    n, d = a_sorted.shape
    accumulate = total is not None
    if accumulate and (total.dtype != torch.float64 or total.numel() != 1 or total.device != a_sorted.device):
        raise RuntimeError("swd_pair_loss: total must be one float64 value on the projections' device")
    if not accumulate:
        total = torch.empty(1, dtype=torch.float64, device=a_sorted.device)
    ws = torch.empty(_scratch("vcg_swd_pair_loss_workspace", n, d) // 4, dtype=torch.float32, device=a_sorted.device)
    gproj = torch.empty((d, n), dtype=torch.float32, device=a_sorted.device)
    out = torch.empty((), dtype=torch.float32, device=a_sorted.device)
    _call("vcg_swd_pair_loss", _ptr(a_sorted), _ptr(b_sorted), _ptr(perm_a), _ptr(gproj), n, d, float(weight), int(accumulate),
          _ptr(total), _ptr(out), _ptr(ws), ws.numel() * 4, _stream())
    return out, gproj, total


def swd_unit_columns(x):
    """A contiguous (K, D) matrix with every column scaled to unit 2-norm (the sum of squares in double)."""
    _require_gpu(x, "swd_unit_columns")
    if x.dim() != 2 or not x.is_contiguous() or x.numel() == 0:
        raise RuntimeError(f"swd_unit_columns: expected a contiguous (K, D) matrix, got shape {tuple(x.shape)}")
    out = torch.empty_like(x)
    _call("vcg_swd_unit_columns", _ptr(x), _ptr(out), x.shape[0], x.shape[1], _stream())
    return out


def swd_loss_geometry(n_images, h, w, levels):
    """[(H_k, W_k, s_k, n_k)] of the `levels` levels of the loss on `n_images` H x W images; refuses more levels than the image has."""
    levels = _swd_int(levels, "levels", "swd_loss")
    if not 1 <= levels <= SWD_LOSS_MAX_LEVELS:
        raise RuntimeError(f"swd_loss: levels must be an integer in 1..{SWD_LOSS_MAX_LEVELS}, got {levels}")
    have = swd_loss_levels(h, w)
    if levels > have:
        raise RuntimeError(f"swd_loss: {levels} levels asked of {h}x{w} images, which have {have} (a level's sides are even halves "
                           "of at least 16)")
    out = []
    for k in range(levels):
        hk, wk = h >> k, w >> k
        s = swd_cell_side(n_images, hk, wk)
        out.append((hk, wk, s, n_images * (hk // s) * (wk // s)))
    return out


class _SwdLossFn(torch.autograd.Function):
    """The stage calls of `swd_loss` chained.  Kept for the backward: gproj (D, n_k) per level, the directions and the geometry —
    no image."""

    @staticmethod
    def forward(ctx, a, b, levels, offsets, dirs):
        la, lb = as_phys(a), as_phys(b)
        n_img, h, w = la.shape[:3]
        geom, kept, out, total = [], [], None, None
        for k, (hk, wk, s, n) in enumerate(swd_loss_geometry(n_img, h, w, levels)):
            if k:
                la, lb = swd_pool(la), swd_pool(lb)
            oy, ox = offsets[k]
            pa = swd_project(swd_grid_gather(la, s, oy, ox), dirs)
            pb = swd_project(swd_grid_gather(lb, s, oy, ox), dirs)
            ka, ra = sort_columns_indexed(pa)
            out, gproj, total = swd_pair_loss(ka, sort_columns(pb), ra, 1.0 / levels, total)
            kept.append(gproj)
            geom.append((hk, wk, s, int(oy), int(ox), n))
        ctx.save_for_backward(dirs, *kept)
        ctx.geom = (n_img, levels, tuple(geom))
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        n_img, levels, geom = ctx.geom
        dirs, *kept = ctx.saved_tensors
        g = g.contiguous()
        coarser = None
        for (hk, wk, s, oy, ox, n), gproj in zip(reversed(geom), reversed(kept)):
            gdesc = swd_project(dirs, gproj).t()          # (n, 147): the projection with the roles swapped
            ga = swd_grid_scatter(gdesc, (n_img, hk, wk), s, oy, ox, 1.0 / (n * dirs.shape[1] * levels), g)
            if coarser is not None:
                swd_pool_adjoint_add(coarser, ga)
            coarser = ga
        return logical_of(coarser, 3), None, None, None, None


def swd_loss(generated, target, levels, plan):
    """Sliced Wasserstein distance between the 7x7x3 patch sets of `generated` and `target`, (N, 3, H, W) images with H, W >= 16,
    over `levels` in 1..3 levels of a 2 x 2 box pyramid: per level one patch per s x s cell at the plan's offset, projected on
    the plan's 128 unit directions, every direction sorted, mean |sorted generated - sorted target|; the mean over the levels,
    a 0-dim fp32 tensor.  `plan`: SwdPlan.  `target` takes no gradient."""
    if target.requires_grad:
        raise RuntimeError("swd_loss: the target must not require a gradient (only d loss / d generated is computed)")
    if generated.shape != target.shape:
        raise RuntimeError(f"swd_loss: shape mismatch {tuple(generated.shape)} vs {tuple(target.shape)}")
    if generated.dim() != 4 or generated.shape[1] != 3:
        raise RuntimeError(f"swd_loss: expected (N, 3, H, W) images, got shape {tuple(generated.shape)}")
    _require_gpu(generated, "swd_loss")
    _require_gpu(target, "swd_loss")
    geom = swd_loss_geometry(generated.shape[0], generated.shape[2], generated.shape[3], levels)
    offsets, dirs = plan
    _require_gpu(dirs, "swd_loss")
    if tuple(dirs.shape) != (SWD_DESC, SWD_LOSS_DIRS) or not dirs.is_contiguous() or dirs.requires_grad:
        raise RuntimeError(f"swd_loss: the plan's directions must be a contiguous ({SWD_DESC}, {SWD_LOSS_DIRS}) matrix without a "
                           f"gradient, got shape {tuple(dirs.shape)}")
    if len(offsets) != len(geom):
        raise RuntimeError(f"swd_loss: the plan holds {len(offsets)} offsets for {len(geom)} levels")
    offsets = tuple((_swd_int(oy, "oy", "swd_loss"), _swd_int(ox, "ox", "swd_loss")) for oy, ox in offsets)
    for (oy, ox), (_, _, s, _) in zip(offsets, geom):
        if not (0 <= oy <= s - SWD_PATCH and 0 <= ox <= s - SWD_PATCH):
            raise RuntimeError(f"swd_loss: offset ({oy}, {ox}) outside [0, {s - SWD_PATCH}] of a {s}x{s} cell")
    return _SwdLossFn.apply(generated, target, int(levels), offsets, dirs)
