"""CPU: the attention entries with log-sum-exp and the backward (include/cln_amd_ext.h: cln_fa2_fwd_lse, cln_fa2_fwd_causal_lse, cln_fa2_bwd,
cln_fa2_bwd_causal; csrc/flash_attn_m16x_ext.hip, csrc/flash_attn_bwd.hip) -- header, exports, argument checks before any device access,
cln_describe texts, "linked == plannable" for the LSE forwards (fa2_fwd_m16x_kernel with LSE) and the fa2b:: backward kernels, and their code (16x16x32 f16 MFMAs only, no spill, no scratch, no MFMA
writing over its own operands). No GPU needed: hipcc cross-compiles."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cln_amd_ext.h")
CSRC = os.path.join(ROOT, "cuda-learn-notes_amd", "csrc")
SINGLE = " [single stage: every tile fetch waited for where it is issued]"
FWD = ("cln_fa2_fwd_lse", "cln_fa2_fwd_causal_lse")
BWD = ("cln_fa2_bwd", "cln_fa2_bwd_causal")
sys.path.insert(0, os.path.join(ROOT, "cuda-learn-notes_amd", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_handles import M16X, M16X_CLAIMS, kernel_handles, m16x_args  # noqa: E402


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_standalone(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*f1)(const void*, const void*, const void*, void*, float*, int, int, int, int, int, void*) = cln_fa2_fwd_lse;\n"
                   "int (*f2)(const void*, const void*, const void*, void*, float*, int, int, int, int, int, void*) = cln_fa2_fwd_causal_lse;\n"
                   "int (*b1)(const void*, const void*, const void*, const void*, const void*, const float*, float*, void*, void*, void*,"
                   " int, int, int, int, void*) = cln_fa2_bwd;\n"
                   "int (*b2)(const void*, const void*, const void*, const void*, const void*, const float*, float*, void*, void*, void*,"
                   " int, int, int, int, void*) = cln_fa2_bwd_causal;\n"
                   "int main(void) { return f1 && f2 && b1 && b2 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _fn(name):
    from cuda_learn_notes_amd import _loader
    fn = getattr(ctypes.CDLL(_loader.so_path("libcln_amd.so")), name)
    if name in FWD:
        fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    else:
        fn.argtypes = [ctypes.c_void_p] * 10 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def test_product_library_exports_the_entries(built):
    from cuda_learn_notes_amd import _loader
    lib = ctypes.CDLL(_loader.so_path("libcln_amd.so"))
    for n in FWD + BWD:
        assert hasattr(lib, n), n
    for n in ("fa2_fwd_lse", "fa2_bwd", "fa2_attention"):
        assert hasattr(built, n), n


@pytest.mark.parametrize("name", FWD)
def test_lse_entries_check_arguments_before_any_device_access(built, name):
    f = _fn(name)
    q, k, v, o, l = (0x10000 * (i + 1) for i in range(5))  # never dereferenced: every call below fails its checks first
    assert f(None, k, v, o, l, 1, 1, 256, 64, 2, None) == -1
    assert f(q, k, v, o, None, 1, 1, 256, 64, 2, None) == -1
    assert f(q, k, v, o, l + 4, 1, 1, 256, 64, 2, None) == -1  # misaligned
    assert f(q + 2, k, v, o, l, 1, 1, 256, 64, 2, None) == -1
    assert f(q, k, v, q, l, 1, 1, 256, 64, 2, None) == -1  # output == input
    assert f(q, k, v, o, v, 1, 1, 256, 64, 2, None) == -1
    for dims in ((0, 1, 256, 64), (1, 0, 256, 64), (1, 1, 0, 64), (1, 1, 256, 0), (-1, 1, 256, 64)):
        assert f(q, k, v, o, l, *dims, 2, None) == -1, dims
    for D in (32, 96, 256, 512):
        assert f(q, k, v, o, l, 1, 8, 256, D, 2, None) == -2, D
    for N in (64, 128, 320, 1000, 4096 + 128):
        assert f(q, k, v, o, l, 1, 8, N, 128, 1, None) == -2, N
    assert f(q, k, v, o, l, 65536, 65536, 256, 64, 2, None) == -2  # grid size


@pytest.mark.parametrize("name", BWD)
def test_bwd_entries_check_arguments_before_any_device_access(built, name):
    f = _fn(name)
    p = [0x10000 * (i + 1) for i in range(10)]  # q, k, v, o, dout, lse, delta, dq, dk, dv: never dereferenced
    for i in range(10):
        a = list(p)
        a[i] = None
        assert f(*a, 1, 1, 256, 64, None) == -1, i
        a[i] = p[i] + 8
        assert f(*a, 1, 1, 256, 64, None) == -1, i
    for out in range(6, 10):
        for src in range(10):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, 1, 1, 256, 64, None) == -1, (out, src)
    for dims in ((0, 1, 256, 64), (1, 0, 256, 64), (1, 1, 0, 64), (1, 1, 256, 0), (1, -2, 256, 64)):
        assert f(*p, *dims, None) == -1, dims
    for D in (32, 96, 256, 512):
        assert f(*p, 1, 8, 256, D, None) == -2, D
    for N in (64, 128, 320, 1000, 4096 + 128):
        assert f(*p, 1, 8, N, 128, None) == -2, N
    assert f(*p, 65536, 65536, 256, 64, None) == -2  # grid size


def test_describe_texts_and_stages(built):
    m = built.manifest
    for D in (64, 128):
        for N in (256, 512, 4096):
            for st in (1, 2, 3):
                for name in FWD:
                    t = m.describe(name, (2, 32, N, D), st)
                    assert t.startswith("fa2_fwd_m16x_lse<D=%d," % D), t
                    assert t.endswith(SINGLE) == (st == 1), t
                    assert ("key <= query" in t) == (name == "cln_fa2_fwd_causal_lse"), t
                    assert m.stages_honoured(name, (2, 32, N, D), st)
                for name in BWD:
                    t = m.describe(name, (2, 32, N, D), st)
                    assert t.startswith("fa2_bwd_dq<D=%d," % D) and "then fa2_bwd_dkdv<D=%d," % D in t, t
                    assert "stages ignored" in t and "deterministic" in t, t
                    assert ("key <= query" in t) == (name == "cln_fa2_bwd_causal"), t
                    assert not m.stages_honoured(name, (2, 32, N, D), st)
    for dims in ((1, 8, 256, 32), (1, 8, 256, 96), (1, 8, 256, 256), (1, 8, 384, 64), (1, 8, 128, 128)):
        for name in FWD + BWD:
            with pytest.raises(ValueError):
                m.describe(name, dims, 2)


def test_new_names_stay_off_the_reference_surface(built):
    m = built.manifest
    names = {e.name for e in m.ENTRIES}
    for n in FWD + BWD:
        assert n not in names and n.replace("cln_", "") not in names
    gen = open(os.path.join(ROOT, "include", "cln_amd.h")).read()
    assert not any(n + "(" in gen for n in FWD + BWD)


def test_fa2b_kernels_in_the_product_library_are_exactly_the_plannable_ones(built):
    from cuda_learn_notes_amd import _loader
    linked = set()
    for fam, a in kernel_handles(_loader.so_path("libcln_amd.so")):
        if fam == M16X and M16X_CLAIMS["lse"](a):
            # <D, rows per wave, key tile, fragment prefetch depth, deferred key blocks, option bits (5; + 32768 + 2 << 16: single stage), V as [B,H,N,D],
            # causal, launch order (1: heaviest first), LSE>
            causal = a[7] == "true"
            assert a[1:3] == ["32", "128"] and a[6] == "false", a
            assert a[3:5] == (["8", "4"] if a[0] == "64" else ["4", "4"]) and a[5] in ("5", "163845"), a
            assert a[8] == ("1" if causal else "0"), a
            linked.add(("fwd", int(a[0]), causal, a[5] == "163845"))
        elif fam.startswith("fa2b::"):
            assert fam in ("fa2b::fa2_bwd_dq_kernel", "fa2b::fa2_bwd_dkdv_kernel"), fam
            linked.add((fam.split("::")[1], int(a[0]), a[-1] == "true", None))
    plannable = set()
    for D in (32, 64, 96, 128, 256):
        for (B, H) in ((1, 1), (1, 8), (2, 96)):
            for N in (128, 256, 512, 4096):
                for st in (1, 2):
                    for name in FWD + BWD:
                        try:
                            t = built.manifest.describe(name, (B, H, N, D), st)
                        except ValueError:
                            continue
                        causal = "key <= query" in t
                        if name in FWD:
                            plannable.add(("fwd", int(re.match(r"fa2_fwd_m16x_lse<D=(\d+),", t).group(1)), causal, "single stage" in t))
                        else:
                            for k in re.findall(r"(fa2_bwd_dq|fa2_bwd_dkdv)<D=(\d+),", t):
                                plannable.add((k[0] + "_kernel", int(k[1]), causal, None))
    assert len(plannable) == 16, sorted(plannable)
    assert linked == plannable, sorted(linked ^ plannable)


@pytest.mark.parametrize("unit,count", [("flash_attn_m16x_ext.hip", 8), ("flash_attn_bwd.hip", 8)])
def test_fa2b_kernels_use_f16_mfma_only_and_keep_registers(tmp_path, unit, count):
    import kernel_resources as kr
    import mfma_overlap_scan as scan
    kernels, s = kr.report(os.path.join(CSRC, unit), keep=str(tmp_path))
    # the backward kernels (fa2b::) and the forwards that feed them (fa2_fwd_m16x_kernel with LSE; the unit's causal forwards: test_fa2_causal_surface.py)
    ks = [k for k in kernels if "fa2b::" in k["demangled"] or (m16x_args(k["demangled"]) and M16X_CLAIMS["lse"](m16x_args(k["demangled"])))]
    assert len(ks) == count, [k["demangled"] for k in kernels]
    text = open(s).read()
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]  # (a kernel may hold more than one s_endpgm: early exits)
        assert set(re.findall(r"v_mfma_\w+", body)) == {"v_mfma_f32_16x16x32_f16"}, k["demangled"]
        assert "v_pk_add_f32" not in body  # -fno-slp-vectorize on this unit
    assert not scan.scan(text)

