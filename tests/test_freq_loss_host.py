"""CPU: the focal frequency loss's C ABI and binding — what needs no GPU (flags, configure_loss: test_image_terms_host.py)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vcg_freq_loss_workspace", "vcg_freq_loss_spectrum", "vcg_freq_loss_fwd", "vcg_freq_loss_bwd")


def side_cap():
    text = open(os.path.join(ROOT, "include", "vcg.h")).read()
    return int(re.search(r"#define\s+VCG_FREQ_MAX_SIDE\s+(\d+)", text).group(1))


def test_header_exports_and_binding_have_the_four_entries(pkg):
    text = open(os.path.join(ROOT, "include", "vcg.h")).read()
    assert "F_n[j, k] = exp(-2 pi i j k / n) / sqrt(n)" in text            # the formulas are part of the header
    assert "Re(F_H^H (w . D) F_W^H)" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vcg_[a-z0-9_]+)\s*\(", text))
    path = pkg._native.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/vcg.h"
        assert name in exported, f"{name} is not exported by libvcg.so"
        assert name in pkg._native.SIGNATURES, f"{name} is not in the ctypes table"
    assert "freq_loss.hip" in pkg._native.SOURCES
    assert pkg._native.lib().vcg_abi_version() == 6            # the entries are additive
    assert side_cap() >= 1024


def test_size_functions(pkg):
    lib = pkg._native.lib()
    cap = side_cap()

    def err():
        return lib.vcg_last_error().decode()

    for fn in (lib.vcg_freq_loss_workspace, lib.vcg_freq_loss_spectrum):
        assert fn(0, 32, 32) == 0 and "N=0" in err()
        assert fn(1, 0, 32) == 0 and "H=0" in err()
        assert fn(1, 32, -2) == 0 and "W=-2" in err()
        assert fn(1, cap + 1, 32) == 0 and "cap" in err()
        assert fn(1, 32, cap + 1) == 0 and "cap" in err()
        for n, h, w in [(1, 1, 1), (1, 1, 2), (3, 9, 17), (2, 17, 33), (1, 130, 258), (8, 256, 256), (1, cap, cap), (1, 1, cap)]:
            size = fn(n, h, w)
            assert size > 0 and size % 16 == 0, (n, h, w, size)
    # the kept state holds at least the full complex spectrum of every plane; the scratch one more array of that size
    assert lib.vcg_freq_loss_spectrum(8, 256, 256) >= 24 * 256 * 256 * 8
    assert lib.vcg_freq_loss_workspace(8, 256, 256) >= 24 * 256 * 256 * 8


def test_bad_arguments_are_rejected_without_touching_the_gpu(pkg):
    lib = pkg._native.lib()
    buf = (ctypes.c_double * 128)()                             # host memory: only ever inspected as an address
    base = ctypes.addressof(buf)
    base += -base % 16
    P = ctypes.c_void_p
    a, b, out, spec, ws = P(base), P(base + 64), P(base + 128), P(base + 256), P(base + 512)
    cap = side_cap()
    N, H, W = 2, 24, 40
    need, keep = lib.vcg_freq_loss_workspace(N, H, W), lib.vcg_freq_loss_spectrum(N, H, W)
    assert need and keep

    def err():
        return lib.vcg_last_error().decode()

    def fwd(a=a, b=b, out=out, n=N, h=H, w=W, alpha=1.0, spec=spec, keep=keep, ws=ws, need=need):
        return lib.vcg_freq_loss_fwd(a, b, out, n, h, w, alpha, spec, keep, ws, need, None)

    def bwd(spec=spec, keep=keep, gout=out, ga=a, n=N, h=H, w=W, alpha=1.0, ws=ws, need=need):
        return lib.vcg_freq_loss_bwd(spec, keep, gout, ga, n, h, w, alpha, ws, need, None)

    for call in (fwd, bwd):
        assert call(n=0) != 0 and "N=0" in err()
        assert call(n=-3) != 0 and "N=-3" in err()
        assert call(h=0) != 0 and "H=0" in err()
        assert call(w=-1) != 0 and "W=-1" in err()
        assert call(h=cap + 1) != 0 and "cap" in err()
        assert call(w=cap + 1) != 0 and "cap" in err()
        assert call(alpha=-0.5) != 0 and "alpha" in err()
        assert call(alpha=float("nan")) != 0 and "alpha" in err()
        assert call(alpha=float("inf")) != 0 and "alpha" in err()
        assert call(keep=keep - 1) != 0 and "spectrum of" in err() and str(keep) in err()
        assert call(need=need - 1) != 0 and "workspace of" in err() and str(need) in err()
        assert call(spec=None) != 0 and "null pointer" in err()
        assert call(ws=None) != 0 and "null pointer" in err()
        assert call(spec=P(base + 256 + 8)) != 0 and "aligned" in err()
        assert call(ws=P(base + 512 + 4)) != 0 and "aligned" in err()
    for name in ("a", "b", "out"):
        assert fwd(**{name: None}) != 0 and "null pointer" in err()
    assert fwd(a=P(base + 4)) != 0 and "aligned" in err()
    assert fwd(b=P(base + 64 + 8)) != 0 and "aligned" in err()
    assert fwd(out=P(base + 128 + 2)) != 0 and "aligned" in err()
    for name in ("gout", "ga"):
        assert bwd(**{name: None}) != 0 and "null pointer" in err()
    assert bwd(ga=P(base + 8)) != 0 and "aligned" in err()
    assert bwd(gout=P(base + 128 + 1)) != 0 and "aligned" in err()
