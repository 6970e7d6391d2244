"""CPU: the gradient-matching loss's C ABI and binding — what needs no GPU (flags, configure_loss: test_image_terms_host.py)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vcg_grad_loss_workspace", "vcg_grad_loss_fwd", "vcg_grad_loss_bwd")
TILE = 32                                                       # include/vcg.h: one 2 S-slot group per 32 x 32 tile of pixels


def test_header_exports_and_binding_have_the_three_entries(pkg):
    text = open(os.path.join(ROOT, "include", "vcg.h")).read()
    assert "ceil(H / 32) ceil(W / 32) 2 scales doubles" in text          # the workspace formula the next test restates
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vcg_[a-z0-9_]+)\s*\(", text))
    path = pkg._native.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/vcg.h"
        assert name in exported, f"{name} is not exported by libvcg.so"
        assert name in pkg._native.SIGNATURES, f"{name} is not in the ctypes table"
    assert "grad_loss.hip" in pkg._native.SOURCES
    assert pkg._native.lib().vcg_abi_version() == 6            # the entries are additive


def test_workspace_is_two_doubles_per_scale_and_tile(pkg):
    lib = pkg._native.lib()
    shapes = [(1, 1, 1), (3, 27, 1), (2, TILE - 1, TILE + 1), (2, TILE, TILE), (1, TILE + 1, TILE - 1), (2, 2 * TILE + 1, 70),
              (8, 256, 256)]
    for n, h, w in shapes:
        for s in (1, 2, 3, 4):
            tiles = -(-h // TILE) * -(-w // TILE)
            assert lib.vcg_grad_loss_workspace(n, h, w, s) == (n * tiles * 2 * s * 8 + 15) // 16 * 16, (n, h, w, s)
    assert lib.vcg_grad_loss_workspace(8, 256, 256, 4) == 8 * 64 * 8 * 8


def test_bad_arguments_are_rejected_without_touching_the_gpu(pkg):
    lib = pkg._native.lib()
    buf = (ctypes.c_double * 64)()                              # host memory: only ever inspected as an address
    base = ctypes.addressof(buf)
    base += -base % 16
    P = ctypes.c_void_p
    a, b, out, ws = P(base), P(base + 64), P(base + 128), P(base + 256)

    def err():
        return lib.vcg_last_error().decode()

    assert lib.vcg_grad_loss_workspace(0, 32, 32, 4) == 0 and "N=0" in err()
    assert lib.vcg_grad_loss_workspace(1, 0, 32, 4) == 0 and "H=0" in err()
    assert lib.vcg_grad_loss_workspace(1, 32, -2, 4) == 0 and "W=-2" in err()
    assert lib.vcg_grad_loss_workspace(1, 32, 32, 0) == 0 and "scales=0" in err()
    assert lib.vcg_grad_loss_workspace(1, 32, 32, 5) == 0 and "scales=5" in err()
    need = lib.vcg_grad_loss_workspace(2, 32, 32, 4)
    assert need == 2 * 8 * 8
    # forward
    assert lib.vcg_grad_loss_fwd(a, b, out, 0, 32, 32, 4, ws, need, None) != 0 and "N=0" in err()
    assert lib.vcg_grad_loss_fwd(a, b, out, -3, 32, 32, 4, ws, need, None) != 0 and "N=-3" in err()
    assert lib.vcg_grad_loss_fwd(a, b, out, 2, 0, 32, 4, ws, need, None) != 0 and "H=0" in err()
    assert lib.vcg_grad_loss_fwd(a, b, out, 2, 32, -1, 4, ws, need, None) != 0 and "W=-1" in err()
    assert lib.vcg_grad_loss_fwd(a, b, out, 2, 32, 32, 0, ws, need, None) != 0 and "scales=0" in err()
    assert lib.vcg_grad_loss_fwd(a, b, out, 2, 32, 32, 5, ws, need, None) != 0 and "scales=5" in err()
    for nulls in ((None, b, out, ws), (a, None, out, ws), (a, b, None, ws), (a, b, out, None)):
        assert lib.vcg_grad_loss_fwd(nulls[0], nulls[1], nulls[2], 2, 32, 32, 4, nulls[3], need, None) != 0
        assert "null pointer" in err()
    assert lib.vcg_grad_loss_fwd(a, b, out, 2, 32, 32, 4, ws, need - 1, None) != 0
    assert "workspace of" in err() and str(need) in err()
    assert lib.vcg_grad_loss_fwd(a, b, out, 2, 32, 32, 4, P(base + 256 + 8), need, None) != 0 and "aligned" in err()
    assert lib.vcg_grad_loss_fwd(P(base + 4), b, out, 2, 32, 32, 4, ws, need, None) != 0 and "aligned" in err()
    assert lib.vcg_grad_loss_fwd(a, P(base + 64 + 8), out, 2, 32, 32, 4, ws, need, None) != 0 and "aligned" in err()
    # backward
    gout, ga = out, ws
    assert lib.vcg_grad_loss_bwd(a, b, gout, ga, 0, 32, 32, 4, None) != 0 and "N=0" in err()
    assert lib.vcg_grad_loss_bwd(a, b, gout, ga, 2, 32, 0, 4, None) != 0 and "W=0" in err()
    assert lib.vcg_grad_loss_bwd(a, b, gout, ga, 2, -7, 32, 4, None) != 0 and "H=-7" in err()
    assert lib.vcg_grad_loss_bwd(a, b, gout, ga, 2, 32, 32, 0, None) != 0 and "scales=0" in err()
    assert lib.vcg_grad_loss_bwd(a, b, gout, ga, 2, 32, 32, 5, None) != 0 and "scales=5" in err()
    for nulls in ((None, b, gout, ga), (a, None, gout, ga), (a, b, None, ga), (a, b, gout, None)):
        assert lib.vcg_grad_loss_bwd(*nulls, 2, 32, 32, 4, None) != 0 and "null pointer" in err()
    assert lib.vcg_grad_loss_bwd(a, b, gout, P(base + 256 + 4), 2, 32, 32, 4, None) != 0 and "aligned" in err()
    assert lib.vcg_grad_loss_bwd(P(base + 8), b, gout, ga, 2, 32, 32, 4, None) != 0 and "aligned" in err()
