"""CPU: the C-ABI library builds for gfx950, loads, and exports exactly what include/vcg.h declares.
No compute call is made here (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "vcg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vcg_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol(pkg):
    path = pkg._native.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert len(syms) >= 30
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f"declared in vcg.h but not exported: {missing}"


def test_no_c_symbol_is_exported_behind_the_headers_back(pkg):
    """Every `vcg_*` function with C linkage in the library is declared in include/vcg.h (internal helpers keep C++ linkage;
    diagnostic hooks are named here)."""
    import subprocess
    path = pkg._native.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("vcg_")})
    diagnostic = {"vcg_debug_set_stamp"}                                   # stamp hook of the -DVCG_STAMP diagnostic build (a no-op here)
    extra = [s for s in exported if s not in header_symbols() and s not in diagnostic]
    assert not extra, f"exported with C linkage but not declared in vcg.h: {extra}"


def test_python_binding_covers_the_header(pkg):
    assert sorted(pkg._native.SIGNATURES) == header_symbols()
    lib = pkg._native.lib()
    assert lib.vcg_abi_version() == 6


def test_code_object_targets_gfx950(pkg):
    path = pkg._native.build()
    blob = open(path, "rb").read()
    assert b"gfx950" in blob
    # the conv kernels must really be on the fp32 matrix core
    tool = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if os.path.exists(tool):
        out = subprocess.run(["bash", "-c", f"cd /tmp && /opt/rocm/lib/llvm/bin/clang-offload-bundler --list --type=o --input={path} 2>/dev/null | head -5"],
                             capture_output=True, text=True).stdout
        assert "gfx950" in out or out == ""


def test_bad_arguments_are_rejected_without_touching_the_gpu(pkg):
    lib = pkg._native.lib()
    cd = (ctypes.c_int32 * 16)()
    cd[0], cd[1], cd[2], cd[3], cd[4] = 1, 8, 8, 3, 8          # Cin pitch 3 is illegal
    cd[5] = cd[6] = 3
    cd[7], cd[8], cd[9], cd[10], cd[12], cd[13] = 1, 1, 1, 1, 3, 8
    assert lib.vcg_conv_wgrad_workspace(cd) == 0
    rc = lib.vcg_conv_fwd(None, None, None, None, cd, None, 0, None)
    assert rc != 0
    assert b"multiple of 4" in lib.vcg_last_error()
    cd[3] = 4
    cd[1] = cd[2] = 1                                           # reflect pad 1 on a 1x1 map is illegal
    assert lib.vcg_conv_fwd(None, None, None, None, cd, None, 0, None) != 0
    assert b"reflect" in lib.vcg_last_error()


def _desc(n, h, w, cin, cout, k, stride=1, pad=1, reflect=1, ups=1, act=0, cin_log=None, cout_log=None):
    cd = (ctypes.c_int32 * 16)()
    cd[0:14] = [n, h, w, cin, cout, k, k, stride, pad, reflect, ups, act, cin_log or cin, cout_log or cout]
    return cd


def test_launch_plans_are_host_side_and_consistent(pkg):
    """Workspace / packed-weight sizes come from the same planners the launches use (no GPU needed): the Winograd
    path is taken exactly for 3x3 stride-1 layers with Kc >= 128, Cout >= 64 on even maps, the kw-folded path for the
    3-channel head, everything else stays on the direct kernels."""
    lib = pkg._native.lib()
    f4 = 4
    # R-block conv: Winograd in all three directions
    r = _desc(8, 16, 16, 1024, 1024, 3)
    T, Tp, kc, co = 8 * 8 * 8, 8 * 9 * 9, 1024, 1024
    # Wf (fp32) + U + Ud: the Winograd-transformed kernels as pre-split fp16 planes (2 pieces x 2 bytes = 1 float per value)
    # + the 16-float header that keeps the kernel's largest magnitude (the planes hold w / s)
    assert lib.vcg_pack_weight_floats(r) == 9 * kc * co + 2 * 16 * kc * co + 16
    assert lib.vcg_conv_fwd_workspace(r) == 16 * T * (kc + co) * f4 + 512
    assert lib.vcg_conv_dgrad_workspace(r) == 16 * Tp * (kc + co) * f4 + 1024       # V and M over the padded domain's 9 x 9 tiles
    assert lib.vcg_conv_wgrad_workspace(r) > 16 * T * (kc + co) * f4                  # transforms + stream-K slabs
    # same channels on an odd map: direct kernels, K-sliced forward (slabs) but no Winograd buffers
    odd = _desc(8, 15, 15, 1024, 1024, 3)
    assert lib.vcg_pack_weight_floats(odd) == lib.vcg_pack_weight_floats(r)           # packing sees no image size
    assert lib.vcg_conv_fwd_workspace(odd) < 16 * 8 * 7 * 7 * (kc + co) * f4
    # D block (folded PixelUnshuffle): Kc = 4 * 128
    d2 = _desc(8, 128, 128, 128, 256, 3, ups=2)
    assert lib.vcg_pack_weight_floats(d2) == 9 * 512 * 256 + 2 * 16 * 512 * 256 + 16
    assert lib.vcg_conv_fwd_workspace(d2) == 16 * (8 * 32 * 32) * (512 + 256) * f4 + 512
    # small channel counts: no transformed copies
    u4 = _desc(8, 256, 256, 32, 64, 3)
    # Wf + the pre-split weight planes of the direct split-operand kernels: WFT [Cout][K/32][2][32] (forward), WFD
    # [(tap, c)][Cout/32][2][32] (data gradient): 32 floats per (row, 32-wide block); + the header
    assert lib.vcg_pack_weight_floats(u4) == 9 * 32 * 64 + 64 * 9 * 32 + 9 * 32 * 2 * 32 + 16
    assert lib.vcg_conv_fwd_workspace(u4) == 0
    # ... and it runs on the LDS-slab kernels: the data gradient over the padded domain (H + 2) x (W + 2), folded afterwards
    assert lib.vcg_conv_dgrad_workspace(u4) == 8 * 258 * 258 * 32 * f4 + 256
    # ... and its weight gradient on the row-ring kernel: one [288][64] partial per workgroup + 16 group sums (conv_ring.hip)
    def ring_ws(n, yd, xd, nr, sub=1):
        nseg = (xd + 31) // 32
        nrs = max(768 // (n * nseg * sub), 1)
        rows = max((yd + nrs - 1) // nrs, 8)
        nwg = n * nseg * ((yd + rows - 1) // rows)
        per = (nwg + 15) // 16
        return (sub * nwg + sub * ((nwg + per - 1) // per)) * nr * 64 * f4 + 256
    assert 0 <= lib.vcg_conv_wgrad_workspace(u4) - (ring_ws(8, 256, 256, 288) + 255) // 256 * 256 <= 1 << 20     # + bias column sums
    # the latent convs 1024 -> 64: Kc Cout / (Kc + Cout) = 60 is under every Winograd gate (forward 100, data gradient 80):
    # no transformed copies, the planes of the direct split-operand kernels instead
    mu = _desc(8, 16, 16, 1024, 64, 3)
    assert lib.vcg_pack_weight_floats(mu) == 9 * 1024 * 64 + 64 * (9216 // 32) * 32 + 9 * 1024 * 2 * 32 + 16
    # decoder head 64 -> 3 (pitch 4), 7x7: Wf + the kw-folded copy [(kh, c)][32]; P buffer over the padded columns
    head = _desc(8, 256, 256, 64, 4, 7, pad=3, cout_log=3)
    # (+ that copy's pre-split planes [32][7 * 64 / 32][2][32] for the LDS-slab column kernel, + the header)
    assert lib.vcg_pack_weight_floats(head) == ((49 * 64 * 4 + 63) // 64) * 64 + 7 * 64 * 32 + 7 * 64 * 32 + 16
    assert lib.vcg_conv_fwd_workspace(head) == 8 * 256 * (256 + 6) * 32 * f4 + 256
    # its weight gradient: the ring kernel over the PADDED input pixels (262 x 262), 7 tap rows x 32 columns per partial
    assert 0 <= lib.vcg_conv_wgrad_workspace(head) - (ring_ws(8, 262, 262, 224) + 255) // 256 * 256 <= 1 << 20
    # encoder stem 3 -> 64: the data gradient takes the folded path (padded-domain dxp + P), the forward does not
    stem = _desc(8, 256, 256, 4, 64, 7, pad=3, cin_log=3)
    assert lib.vcg_pack_weight_floats(stem) == ((49 * 4 * 64 + 63) // 64) * 64 + 7 * 64 * 32 + 7 * 64 * 32 + 64 * 7 * 32 + 16     # K = 196 -> 7 blocks
    assert lib.vcg_conv_dgrad_workspace(stem) >= 8 * 262 * 262 * 4 * f4 + 8 * 262 * (256 + 12) * 32 * f4
    # stride-2 discriminator conv: direct everywhere; forward and data gradient may slice K (whole output- / input-sized
    # slabs; the data gradient's blockIdx.z enumerates parity class + 4 x slice)
    disc = _desc(8, 128, 128, 64, 128, 4, stride=2, pad=1)
    assert lib.vcg_pack_weight_floats(disc) == 16 * 64 * 128 + 128 * 32 * 32 + 16 * 64 * 4 * 32 + 16
    assert (lib.vcg_conv_fwd_workspace(disc) - 256) % (8 * 64 * 64 * 128 * f4) in (0, (8 * 64 * 64 * 128 * f4) - 256)
    assert lib.vcg_conv_dgrad_workspace(disc) % (8 * 128 * 128 * 64 * f4) in (0, 256)


def test_product_path_refuses_cpu_tensors(pkg):
    m = pkg.Networks.S(4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 4, 4, 4))
    with pytest.raises(RuntimeError):
        pkg.optim.FusedAdam(m.parameters(), lr=1e-3)


def test_instance_norm_cases_hit_every_ragged_plan(pkg):
    """tests/test_gpu_norm_misc.py mirrors vcg_norm_plan (csrc/vcg_common.h) in Python: the mirror must agree with the plan the
    library sizes its workspace by (ws = N nchunk C 20 + N C 8 + 512 bytes exposes nchunk), and the InstanceNorm case list must
    keep hitting the ragged parts of the plan: the model's layers all split evenly, so a plan change could silently turn the edge
    cases into easy ones."""
    from test_gpu_norm_misc import IN_SHAPES, norm_plan, plan_edges
    lib = pkg._native.lib()
    for N, H, W, C in IN_SHAPES:
        HW = H * W
        ws = lib.vcg_in_workspace(N, HW, C)
        assert (ws - 512 - N * C * 8) % (N * C * 20) == 0, (N, H, W, C, ws)
        assert (ws - 512 - N * C * 8) // (N * C * 20) == norm_plan(N, HW, C)["nchunk"], (N, H, W, C)
    hit = {}
    for N, H, W, C in IN_SHAPES:
        for k, v in plan_edges(N, H * W, C).items():
            hit[k] = hit.get(k, False) or v
    missing = [k for k, v in hit.items() if not v]
    assert not missing, f"no InstanceNorm case runs: {missing}"


def _plan_sweep():
    """a few hundred geometries across the plans' conditions: channels 4..2048, k 1/3/4/7, stride 1/2, ups 1/2, reflect / zero,
    maps 2..256, N 1..16, logical channels below the pitch"""
    import random
    from test_gpu_conv_plans import desc
    rng = random.Random(20261016)
    out = []
    while len(out) < 400:
        k = rng.choice([1, 3, 4, 7])
        s = rng.choice([1, 2])
        ups = rng.choice([1, 2]) if s == 1 else 1
        cin = rng.choice([4, 8, 16, 32, 64, 128, 192, 256, 512, 1024, 2048])
        cout = rng.choice([4, 8, 32, 64, 128, 192, 256, 512, 1024, 2048])
        hl = rng.choice([2, 3, 4, 5, 6, 7, 8, 12, 16, 17, 20, 32, 64, 66, 128, 256])
        wl = hl if rng.random() < 0.8 else rng.choice([3, 6, 9, 16, 64])
        pad = {1: 0, 3: 1, 4: 1, 7: 3}[k]
        refl = rng.choice([0, 1])
        if refl and (pad >= hl or pad >= wl) or hl + 2 * pad < k or wl + 2 * pad < k:
            continue
        cin_log = cin if rng.random() < 0.7 else cin - rng.choice([1, 2, 3])
        cout_log = cout if rng.random() < 0.7 else cout - 1
        out.append(desc(rng.choice([1, 2, 3, 4, 8, 16]), hl * ups, wl * ups, cin, cout, k, s, pad, refl, ups, rng.choice(range(5)),
                        cin_log, cout_log))
    return out


def test_conv_plan_mirror_matches_the_library_and_cases_hit_every_branch(pkg):
    """tests/test_gpu_conv_plans.py mirrors the convolution dispatch (conv_plan).  Without a GPU the library reports the sizes its
    planners (plan_fwd, plan_dgrad, plan_wgrad, pack_layout) derive — forward, forward-with-statistics, data and weight gradient
    workspaces, packed-weight floats, whether Wf is read, saved floats, whether the normalising gather exists — which encode the
    K-slice, Winograd, slab, ring, thin and swapped choices: the mirror must give the same numbers for the GPU case list and a
    sweep of 400 geometries.  And the case list must keep reaching every branch
    of the module's table: a plan change that turns an edge case into an easy one fails here, naming the branch."""
    from test_gpu_conv_plans import CASES, REQUIRED, branch_labels, case_desc, library_sizes, mirror_sizes
    lib = pkg._native.lib()
    cds = [case_desc(c) for c in CASES] + _plan_sweep()
    for cd in cds:
        assert lib.vcg_pack_weight_floats(cd) > 0, (list(cd), lib.vcg_last_error())
        got, want = library_sizes(lib, cd), mirror_sizes(cd)
        assert got == want, f"descriptor {list(cd)[:14]}: library {got} mirror {want}"
    hit = set()
    for c in CASES:
        hit |= branch_labels(case_desc(c), c[2])
    missing = [r for r in REQUIRED if r not in hit]
    assert not missing, f"no convolution case reaches: {missing}"


# what a child process prints: the host-side sizes of every descriptor it is given, then vcg_in_workspace of three shapes
_SIZES_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
job = json.load(sys.stdin)
for name in ("vcg_pack_weight_floats", "vcg_conv_fwd_workspace", "vcg_conv_dgrad_workspace", "vcg_conv_wgrad_workspace",
             "vcg_conv_saved_floats", "vcg_in_workspace"):
    getattr(lib, name).restype = ctypes.c_size_t
lib.vcg_conv_reads_wf.restype = ctypes.c_int
lib.vcg_in_workspace.argtypes = [ctypes.c_int] * 3
for d in job["descs"]:
    cd = (ctypes.c_int32 * 16)(*d)
    print(d[:14], lib.vcg_pack_weight_floats(cd), lib.vcg_conv_fwd_workspace(cd), lib.vcg_conv_dgrad_workspace(cd),
          lib.vcg_conv_wgrad_workspace(cd), lib.vcg_conv_saved_floats(cd), lib.vcg_conv_reads_wf(cd))
for n, hw, c in job["norms"]:
    print("in", n, hw, c, lib.vcg_in_workspace(n, hw, c))
"""
# the kernel-variant switches libvcg.so once read, each at its former non-default value
_RETIRED_SWITCHES = dict(VCG_GEMM_DMA="0", VCG_GEMM_SPREAD="0", VCG_GEMM_SHAPE="32", VCG_GEMM_STAGGER="0", VCG_WINO_PLANES="0",
                         VCG_WINO_GATE_F="1", VCG_WINO_GATE_D="1", VCG_WINO_GATE_W="1", VCG_WGRAD_TR="0", VCG_IN_TAIL="1",
                         VCG_IN_BWD_FLAT="1", VCG_THININ="2", VCG_PLAN_TSCALE="0.25", VCG_SLAB="0", VCG_RING="0")


def test_library_ignores_environment(pkg):
    """libvcg.so reads no environment variable: two fresh processes, one with none of the retired kernel-variant switches set and
    one with every one of them at its former non-default value, report the same pack, workspace and saved sizes for every
    descriptor of the convolution case list and the same InstanceNorm workspaces (the Winograd gates, the slab switch and the
    thin-input mode all used to move these numbers)."""
    import json
    import sys
    from test_gpu_conv_plans import CASES, case_desc
    path = pkg._native.build()
    job = json.dumps({"descs": [list(case_desc(c)) for c in CASES], "norms": [(8, 256 * 256, 64), (8, 16 * 16, 1024), (3, 33 * 17, 36)]})
    clean = {k: v for k, v in os.environ.items() if not k.startswith("VCG_")}
    outs = []
    for env in (clean, dict(clean, **_RETIRED_SWITCHES)):
        res = subprocess.run([sys.executable, "-c", _SIZES_CHILD, path], input=job, env=env, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        outs.append(res.stdout)
    assert len(outs[0].splitlines()) == len(CASES) + 3
    assert outs[0] == outs[1]
