"""CPU: the causal attention entry cln_fa2_fwd_causal (include/cln_amd_ext.h, csrc/flash_attn_m16x_ext.hip) -- header, export, argument
checks before any device access, cln_describe text, "linked == plannable" for its kernels (fa2_fwd_m16x_kernel with CAUSAL and without LSE), and the code of those kernels
(16x16x32 MFMAs only, no spill, no scratch, no MFMA writing over its own operands). No GPU needed: hipcc cross-compiles."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cln_amd_ext.h")
SRC = os.path.join(ROOT, "cuda-learn-notes_amd", "csrc", "flash_attn_m16x_ext.hip")
SINGLE = " [single stage: every tile fetch waited for where it is issued]"
sys.path.insert(0, os.path.join(ROOT, "cuda-learn-notes_amd", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_handles import M16X, M16X_CLAIMS, kernel_handles, m16x_args  # noqa: E402


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_standalone(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*probe_causal)(const void*, const void*, const void*, void*, int, int, int, int, int, void*) = cln_fa2_fwd_causal;\n"
                   "int main(void) { return probe_causal && CLN_ERR_UNSUPPORTED == -2 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    lib = ctypes.CDLL(_loader.so_path("libcln_amd.so"))
    fn = lib.cln_fa2_fwd_causal
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def test_product_library_exports_the_causal_entry(built):
    from cuda_learn_notes_amd import _loader
    assert hasattr(ctypes.CDLL(_loader.so_path("libcln_amd.so")), "cln_fa2_fwd_causal")
    assert hasattr(built, "fa2_fwd_causal")


def test_causal_entry_checks_arguments_before_any_device_access(built):
    f = _lib()
    p = 0x10000  # never dereferenced: every call below fails its checks first
    assert f(None, p, p, p, 1, 1, 256, 64, 2, None) == -1
    assert f(p, p, p, None, 1, 1, 256, 64, 2, None) == -1
    assert f(p + 2, p, p, p, 1, 1, 256, 64, 2, None) == -1  # misaligned
    for dims in ((0, 1, 256, 64), (1, 0, 256, 64), (1, 1, 0, 64), (1, 1, 256, 0), (-1, 1, 256, 64)):
        assert f(p, p, p, p, *dims, 2, None) == -1, dims
    for D in (32, 96, 256, 512):
        for st in (1, 2):
            assert f(p, p, p, p, 1, 8, 256, D, st, None) == -2, D
    for N in (64, 128, 320, 1000, 4096 + 128):
        assert f(p, p, p, p, 1, 8, N, 128, 2, None) == -2, N


def test_describe_names_the_causal_family(built):
    m = built.manifest
    for D in (64, 128):
        for N in (256, 512, 4096):
            for st in (1, 2, 3):
                t = m.describe("cln_fa2_fwd_causal", (2, 32, N, D), st)
                assert t.startswith("fa2_fwd_m16x_causal<D=%d," % D), t
                assert t.endswith(SINGLE) == (st == 1), t
                assert m.stages_honoured("cln_fa2_fwd_causal", (2, 32, N, D), st)
    for dims in ((1, 8, 256, 32), (1, 8, 256, 96), (1, 8, 256, 256), (1, 8, 256, 512), (1, 8, 384, 64), (1, 8, 128, 128)):
        with pytest.raises(ValueError):
            m.describe("cln_fa2_fwd_causal", dims, 2)


def test_causal_kernels_in_the_product_library_are_exactly_the_plannable_ones(built):
    from cuda_learn_notes_amd import _loader
    linked = set()
    for fam, a in kernel_handles(_loader.so_path("libcln_amd.so")):
        if fam != M16X or not M16X_CLAIMS["causal"](a):
            continue
        # <D, rows per wave, key tile, fragment prefetch depth, deferred key blocks, option bits (5 = phase-A priority + split prologue; + 32768 + 2 << 16:
        # single stage), V as [B,H,N,D], CAUSAL, launch order (1: heaviest first), no LSE>
        assert a[1:3] == ["32", "128"] and a[6] == "false", a
        assert a[3:5] == (["8", "4"] if a[0] == "64" else ["4", "4"]) and a[5] in ("5", "163845") and a[8] == "1", a
        linked.add((int(a[0]), a[5] == "163845"))
    plannable = set()
    for D in (32, 64, 96, 128, 256):
        for (B, H) in ((1, 1), (1, 8), (4, 8), (2, 96)):
            for N in (128, 256, 512, 4096):
                for st in (1, 2):
                    try:
                        t = built.manifest.describe("cln_fa2_fwd_causal", (B, H, N, D), st)
                    except ValueError:
                        continue
                    plannable.add((int(re.match(r"fa2_fwd_m16x_causal<D=(\d+),", t).group(1)), "single stage" in t))
    assert plannable == {(64, False), (64, True), (128, False), (128, True)}
    assert linked == plannable, sorted(linked ^ plannable)


def test_causal_kernels_use_16x16x32_mfma_only_and_keep_registers(tmp_path):
    import kernel_resources as kr
    import mfma_overlap_scan as scan
    kernels, s = kr.report(SRC, keep=str(tmp_path))
    ks = [k for k in kernels if m16x_args(k["demangled"]) and M16X_CLAIMS["causal"](m16x_args(k["demangled"]))]
    assert len(ks) == 4, [k["demangled"] for k in kernels]
    text = open(s).read()
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index("s_endpgm")]
        assert set(re.findall(r"v_mfma_\w+", body)) == {"v_mfma_f32_16x16x32_f16"}, k["demangled"]
        assert "v_pk_add_f32" not in body  # -fno-slp-vectorize on this unit
    assert not scan.scan(text)
