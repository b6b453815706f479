"""CPU: the bf16 entries of the paged KV-cache path (include/cln_amd_ext.h: cln_kv_append_paged_varlen_bf16, cln_fa2_prefill_paged_varlen_bf16,
cln_fa2_decode_paged_multi_bf16 with their plan / describe entries; csrc/*_bf16.{cuh,hip}, csrc/paged_bf16.cuh) -- header, exports, the plan
against the fp16 plan, the describe texts against their Python mirrors (tests/paged_bf16_reference.py), every status code before any device
access, the Python entries' dtype message, and the kernels' code: the bf16 MFMA on both products, round-to-nearest-even conversions, nothing
through fp16, no spill, no scratch, the registers of the fp16 siblings. No GPU needed: hipcc cross-compiles."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cln_amd_ext.h")
CSRC = os.path.join(ROOT, "cuda-learn-notes_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "cuda-learn-notes_amd", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_decode_reference as mr  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402

APPEND, APPEND_D = "cln_kv_append_paged_varlen_bf16", "cln_kv_append_paged_varlen_bf16_describe"
PREFILL, PREFILL_D = "cln_fa2_prefill_paged_varlen_bf16", "cln_fa2_prefill_paged_varlen_bf16_describe"
MULTI, MULTI_P, MULTI_D = "cln_fa2_decode_paged_multi_bf16", "cln_fa2_decode_paged_multi_bf16_plan", "cln_fa2_decode_paged_multi_bf16_describe"
NAMES = (APPEND, APPEND_D, PREFILL, PREFILL_D, MULTI, MULTI_P, MULTI_D)
LDS_PER_CU = 160 * 1024


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_seven_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a1)(const void*, const void*, const void*, const int*, const int*, const int*, void*, float*, int, int, int, int, int,"
                   " int, int, int, void*) = %s;\n"
                   "int (*t1)(int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int (*a2)(const void*, const void*, void*, void*, const int*, const int*, const int*, const void*, void*, const float*, int,"
                   " int, int, int, int, int, int, int, int, int, void*) = %s;\n"
                   "int (*t2)(int, int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int (*a3)(const void*, const void*, const void*, const int*, const int*, void*, float*, void*, long long, int, int, int, int,"
                   " int, int, int, int, void*) = %s;\n"
                   "int (*p3)(int, int, int, int, int, int, int, int*, int*, long long*) = %s;\n"
                   "int (*t3)(int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int main(void) { return a1 && t1 && a2 && t2 && a3 && p3 && t3 ? 0 : 1; }\n"
                   % (PREFILL, PREFILL_D, APPEND, APPEND_D, MULTI, MULTI_P, MULTI_D))
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _fn(name, argtypes):
    fn = getattr(_lib(), name)
    fn.argtypes, fn.restype = argtypes, ctypes.c_int
    return fn


def _prefill():
    return _fn(PREFILL, [ctypes.c_void_p] * 8 + [ctypes.c_int] * 8 + [ctypes.c_void_p])


def _append():
    return _fn(APPEND, [ctypes.c_void_p] * 10 + [ctypes.c_int] * 10 + [ctypes.c_void_p])


def _multi():
    return _fn(MULTI, [ctypes.c_void_p] * 8 + [ctypes.c_longlong] + [ctypes.c_int] * 8 + [ctypes.c_void_p])


def _plan(name, *dims):
    fn = _fn(name, [ctypes.c_int] * 7 + [ctypes.c_void_p] * 3)
    s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    rc = fn(*dims, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
    return rc, (s.value, c.value, w.value)


def _describe(name, *dims):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(1280)
    rc = fn(*dims, buf, 1280)
    return rc, buf.value.decode()


def test_library_header_and_package_hold_the_entries(built):
    lib, hdr = _lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ("kv_append_paged_varlen_bf16", "fa2_prefill_paged_varlen_bf16", "fa2_decode_paged_multi_bf16", "fa2_decode_paged_multi_bf16_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    for n in ("describe_prefill_paged_varlen_bf16", "describe_kv_append_paged_varlen_bf16", "describe_decode_paged_multi_bf16"):
        assert hasattr(built.manifest, n), n
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:  # none of the new names is a manifest name
        assert n not in names and n.replace("cln_", "") not in names


def test_plan_is_the_fp16_plan(built):
    """cln_fa2_decode_paged_multi_bf16_plan returns exactly what cln_fa2_decode_paged_multi_plan returns, status and all three numbers, over
    supported, unsupported and invalid arguments; and the Python entries agree with each other and with the mirror."""
    n = 0
    for B in (1, 2, 7, 64, 1024, 4096):
        for T in (1, 3, 8, 9):
            for (Hq, Hkv) in ((1, 1), (8, 2), (32, 8), (8, 1), (6, 2), (8, 3)):
                for (mp, page) in ((1, 16), (19, 16), (256, 16), (1024, 16), (16, 256), (40, 48), (1 << 23, 256)):
                    for D in (64, 128, 96):
                        a = _plan("cln_fa2_decode_paged_multi_plan", B, T, Hq, Hkv, mp, page, D)
                        b = _plan(MULTI_P, B, T, Hq, Hkv, mp, page, D)
                        assert a == b, (B, T, Hq, Hkv, mp, page, D, a, b)
                        if a[0] == 0:
                            assert built.fa2_decode_paged_multi_bf16_plan(B, T, Hq, Hkv, mp, page, D) == a[1] == mr.plan(B, T, Hq, Hkv, mp, page, D)
                            assert built.fa2_decode_paged_multi_plan(B, T, Hq, Hkv, mp, page, D) == a[1]
                            n += 1
    assert n > 300
    for bad in ((0, 1, 8, 2, 4, 16, 64), (1, 0, 8, 2, 4, 16, 64), (1, 1, 8, 2, 0, 16, 64), (1, 1, 0, 2, 4, 16, 64)):
        assert _plan(MULTI_P, *bad)[0] == _plan("cln_fa2_decode_paged_multi_plan", *bad)[0] == -1
    fn = _fn(MULTI_P, [ctypes.c_int] * 7 + [ctypes.c_void_p] * 3)
    assert fn(1, 1, 8, 2, 256, 16, 128, None, None, None) == 0  # every out-parameter may be null
    assert built.fa2_decode_paged_multi_bf16_plan(1, 1, 1, 1, 256, 16, 128)[0] > 1  # the shape the GPU test splits on
    with pytest.raises(RuntimeError, match=r"fa2_decode_paged_multi_bf16: T 9 not supported"):
        built.fa2_decode_paged_multi_bf16_plan(1, 9, 8, 2, 4, 16, 64)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_bf16: headdim 96"):
        built.fa2_decode_paged_multi_bf16_plan(1, 1, 8, 2, 4, 16, 96)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_bf16: 8 query heads are no multiple of 3 KV heads"):
        built.fa2_decode_paged_multi_bf16_plan(1, 1, 8, 3, 4, 16, 64)


def test_describe_texts_match_the_python_mirrors(built):
    m = built.manifest
    for D in (64, 128):
        for G in pr.GROUPS:
            for page in pr.PAGES:
                for (B, tq, Hkv, mp) in ((1, 1, 1, 1), (5, 204, 1, 32), (3, 258, 2, 40), (65, 2112, 8, 300)):
                    Hq = Hkv * G
                    rc, text = _describe(PREFILL_D, B, tq, Hq, Hkv, mp, page, D)
                    assert rc == len(text) > 0, (rc, text)
                    assert text == m.describe_prefill_paged_varlen_bf16(B, tq, Hq, Hkv, mp, page, D) == br.describe_prefill_text(B, tq, Hq, Hkv, mp, page, D)
                    assert text.startswith("fa2_prefill_paged_varlen_bf16_mfma<D=%d,G=%d> B=%d" % (D, G, B)) and "v_mfma_f32_16x16x32_bf16" in text
                    # the fp16 text with the kernel's new name and the bf16 MFMA, nothing else
                    assert text.replace("_bf16_mfma<", "_mfma<").replace("32_bf16", "32_f16") == m.describe_prefill_paged_varlen(B, tq, Hq, Hkv, mp, page, D)
                    for mode in (0, 1, 2):
                        rc, text = _describe(APPEND_D, B, tq, Hq, Hkv, mp, page, D, mode)
                        assert rc == len(text) > 0, (rc, text)
                        assert text == m.describe_kv_append_paged_varlen_bf16(B, tq, Hq, Hkv, mp, page, D, ("none", "half", "interleaved")[mode])
                        assert text == br.describe_append_text(B, tq, Hq, Hkv, mp, page, D, mode)
                        assert text.replace("_bf16_rows<", "_rows<") == m.describe_kv_append_paged_varlen(B, tq, Hq, Hkv, mp, page, D, mode)
                for (B, T, Hkv, mp) in ((1, 1, 1, 256), (7, 3, 2, 19), (64, 8, 8, 300), (1, 8, 1, 4096)):
                    Hq = Hkv * G
                    rc, text = _describe(MULTI_D, B, T, Hq, Hkv, mp, page, D)
                    assert rc == len(text) > 0, (rc, text)
                    assert text == m.describe_decode_paged_multi_bf16(B, T, Hq, Hkv, mp, page, D) == br.describe_multi_text(B, T, Hq, Hkv, mp, page, D)
                    fp16 = m.describe_decode_paged_multi(B, T, Hq, Hkv, mp, page, D)
                    assert text.replace("multi_bf16_mfma<", "multi<").replace("combine_bf16_rows<", "combine<").replace("32_bf16", "32_f16") == fp16
                    assert ("fa2_decode_combine_bf16_rows<D=%d>" % D in text) == (mr.plan(B, T, Hq, Hkv, mp, page, D)[0] > 1)
    for name, dims in ((PREFILL_D, (1, 1, 8, 2, 4, 16, 64)), (APPEND_D, (1, 1, 8, 2, 4, 16, 64, 1)), (MULTI_D, (1, 1, 8, 2, 4, 16, 64))):
        rc, text = _describe(name, *dims)
        f = getattr(_lib(), name)
        small = ctypes.create_string_buffer(b"\xff" * 24, 24)
        assert f(*dims, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
        assert f(*dims, None, 16) == -1 and f(*dims, small, 0) == -1
    for dims in ((1, 2, 8, 8, 4, 16, 96), (1, 2, 3, 1, 4, 16, 64), (1, 2, 8, 8, 4, 48, 64), (1, 2, 8, 3, 4, 16, 64), (0, 2, 8, 8, 4, 16, 64),
                 (1, 0, 8, 8, 4, 16, 64), (1, 2, 8, 8, 1 << 23, 256, 64), (1, 1 << 28, 8, 1, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_prefill_paged_varlen_bf16(*dims)
    for dims in ((1, 9, 8, 8, 4, 16, 64), (1, 1, 8, 8, 4, 16, 96), (1, 1, 3, 1, 4, 16, 64), (0, 1, 8, 8, 4, 16, 64), (1, 1, 8, 3, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_decode_paged_multi_bf16(*dims)
    for dims in ((1, 1, 8, 8, 4, 16, 96, 1), (1, 1, 8, 8, 4, 48, 64, 1), (1, 1, 8, 3, 4, 16, 64, 1), (0, 1, 8, 8, 4, 16, 64, 1),
                 (1, 0, 8, 8, 4, 16, 64, 1), (1, 1, 8, 8, 4, 16, 64, 3), (1, 1, 8, 8, 4, 16, 64, "neox")):
        with pytest.raises(ValueError):
            m.describe_kv_append_paged_varlen_bf16(*dims)


# q, k_pages, v_pages, block_table, seqlens, cu_q, o, lse: never dereferenced, every call below fails its checks first
PTR = [0x10000 * (i + 1) for i in range(8)]
DIMS = (3, 170, 8, 2, 40, 6, 16, 128)  # B, total_q, Hq, Hkv, P, max_pages, page, D
BAD_D = DIMS[:7] + (96,)               # the same with an unsupported D: what a call that passed every -1 check ends on


def test_prefill_checks_arguments_before_any_device_access(built):
    f = _prefill()
    p = list(PTR)
    assert f(*p, *BAD_D, None) == -2 and f(*p[:7], None, *BAD_D, None) == -2  # with and without lse
    for i in range(7):  # a null required pointer, cu_q among them
        a = list(p)
        a[i] = None
        assert f(*a, *DIMS, None) == -1, i
    for i in (0, 1, 2, 6):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, *DIMS, None) == -1, i
    for i in (3, 4, 5, 7):  # block_table, seqlens, cu_q, lse: 4-byte alignment, and no more than that
        a = list(p)
        a[i] = p[i] + 2
        assert f(*a, *DIMS, None) == -1, i
        a[i] = p[i] + 4
        assert f(*a, *BAD_D, None) == -2, i
    for out in (6, 7):  # an output equal to an input or to the other output
        for src in range(8):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, *DIMS, None) == -1, (out, src)
    for i in range(8):  # each dimension non-positive
        for bad in (0, -2):
            d = list(DIMS)
            d[i] = bad
            assert f(*p, *d, None) == -1, d
    assert f(*p, 3, 170, 8, 3, 40, 6, 16, 128, None) == -1  # Hq % Hkv
    for D in (32, 96, 256, 512):
        assert f(*p, *DIMS[:7], D, None) == -2, D
    for (Hq, Hkv) in ((3, 1), (6, 2), (16, 1), (5, 1)):  # G = 3, 3, 16, 5
        assert f(*p, 3, 170, Hq, Hkv, 40, 6, 16, 128, None) == -2, (Hq, Hkv)
    for page in (1, 8, 48, 100, 512):
        assert f(*p, 3, 170, 8, 2, 40, 6, page, 128, None) == -2, page
    assert f(*p, 3, 170, 8, 2, 40, 1 << 23, 256, 128, None) == -2  # max_pages page = 2^31
    assert f(*p, 1, 1 << 28, 8, 1, 40, 6, 16, 128, None) == -2     # total_q G = 2^31
    assert f(*p, 1 << 24, 1, 8, 8, 40, 6, 16, 64, None) == -2      # the B empty slots count too: 8 x 2^24 workgroups


APTR = [0x10000 * (i + 1) for i in range(10)]  # k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q, q_out, rope_table
ADIMS = (3, 23, 8, 2, 40, 6, 16, 128, 4096)    # B, total_q, Hq, Hkv, P, max_pages, page, D, max_pos
ABAD_D = ADIMS[:7] + (96, 4096)


def _no_rope(p):
    return p[:7] + [None, None, None]


def test_append_checks_arguments_before_any_device_access(built):
    f = _append()
    p = list(APTR)
    assert f(*p, *ABAD_D, 1, None) == -2 and f(*p, *ABAD_D, 2, None) == -2 and f(*_no_rope(p), *ABAD_D, 0, None) == -2
    assert f(*p[:7], None, None, p[9], *ABAD_D, 1, None) == -2  # a rotation of K alone
    for mode in (0, 1, 2):
        base = _no_rope(p) if mode == 0 else list(p)
        for i in range(7):  # a null required pointer, cu_q among them
            a = list(base)
            a[i] = None
            assert f(*a, *ADIMS, mode, None) == -1, (mode, i)
        for i in (0, 1, 2, 3) + ((7, 8) if mode else ()):  # 16-byte alignment
            a = list(base)
            a[i] = base[i] + 8
            assert f(*a, *ADIMS, mode, None) == -1, (mode, i)
        for i in (4, 5, 6) + ((9,) if mode else ()):  # block_table, seqlens, cu_q, rope_table: 4-byte alignment, and no more than that
            a = list(base)
            a[i] = base[i] + 2
            assert f(*a, *ADIMS, mode, None) == -1, (mode, i)
            a[i] = base[i] + 4
            assert f(*a, *ABAD_D, mode, None) == -2, (mode, i)
        for i in range(8):  # each dimension non-positive
            for bad in (0, -2):
                d = list(ADIMS)
                d[i] = bad
                assert f(*base, *d, mode, None) == -1, (mode, d)
        assert f(*base, 3, 23, 8, 3, 40, 6, 16, 128, 4096, mode, None) == -1  # Hq % Hkv
    for i in (7, 8, 9):  # mode 0 takes none of q, q_out, rope_table
        a = _no_rope(p)
        a[i] = p[i]
        assert f(*a, *ADIMS, 0, None) == -1, i
    for mode in (1, 2):
        assert f(*p[:9], None, *ADIMS, mode, None) == -1  # no table
        assert f(*p[:7], p[7], None, p[9], *ADIMS, mode, None) == -1  # q without q_out
        assert f(*p[:7], None, p[8], p[9], *ADIMS, mode, None) == -1  # q_out without q
        for max_pos in (0, -1):
            assert f(*p, *ADIMS[:8], max_pos, mode, None) == -1, max_pos
    a = list(p)  # aliasing: q_out == q passes (the call then ends on the unsupported D), every other equality is -1
    a[8] = p[7]
    assert f(*a, *ABAD_D, 1, None) == -2 and f(*a, *ABAD_D, 2, None) == -2
    for out in (2, 3, 8):
        for src in range(10):
            if src != out and (out, src) != (8, 7):
                a = list(p)
                a[out] = p[src]
                assert f(*a, *ADIMS, 1, None) == -1, (out, src)
    for mode in (-1, 3, 7):
        assert f(*p, *ADIMS, mode, None) == -2, mode
    for D in (32, 96, 256, 512):
        assert f(*p, *ADIMS[:7], D, 4096, 1, None) == -2, D
    for page in (1, 8, 48, 100, 512):
        assert f(*p, *ADIMS[:6], page, 128, 4096, 1, None) == -2, page
    assert f(*p, 3, 23, 8, 2, 40, 1 << 23, 256, 128, 4096, 1, None) == -2  # max_pages page = 2^31
    assert f(*p, 3, 1 << 24, 8, 2, 40, 6, 16, 128, 4096, 1, None) == -2     # 2^24 packed rows: one past a grid dimension of 256-thread workgroups


MPTR = [0x10000 * (i + 1) for i in range(8)]  # q, k_pages, v_pages, block_table, seqlens, o, lse, workspace
MDIMS = (3, 4, 8, 2, 40, 6, 16, 128)          # B, T, Hq, Hkv, P, max_pages, page, D: one split, no workspace needed
MBAD_D = MDIMS[:7] + (96,)
WS = 1 << 30


def test_multi_checks_arguments_before_any_device_access(built):
    f = _multi()
    p = list(MPTR)
    assert f(*p, WS, *MBAD_D, None) == -2 and f(*p[:6], None, None, 0, *MBAD_D, None) == -2  # with and without lse / workspace
    for i in range(6):  # a null required pointer
        a = list(p)
        a[i] = None
        assert f(*a, WS, *MDIMS, None) == -1, i
    for i in (0, 1, 2, 5, 6, 7):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, WS, *MDIMS, None) == -1, i
    for i in (3, 4):  # block_table, seqlens: 4-byte alignment, and no more than that
        a = list(p)
        a[i] = p[i] + 2
        assert f(*a, WS, *MDIMS, None) == -1, i
        a[i] = p[i] + 4
        assert f(*a, WS, *MBAD_D, None) == -2, i
    for out in (5, 6, 7):  # an output equal to an input or to another output
        for src in range(8):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, WS, *MDIMS, None) == -1, (out, src)
    for i in range(8):  # each dimension non-positive
        for bad in (0, -2):
            d = list(MDIMS)
            d[i] = bad
            assert f(*p, WS, *d, None) == -1, d
    assert f(*p, WS, 3, 4, 8, 3, 40, 6, 16, 128, None) == -1  # Hq % Hkv
    for D in (32, 96, 256, 512):
        assert f(*p, WS, *MDIMS[:7], D, None) == -2, D
    for T in (9, 16, 100):
        assert f(*p, WS, 3, T, 8, 2, 40, 6, 16, 128, None) == -2, T
    for (Hq, Hkv) in ((3, 1), (6, 2), (16, 1)):
        assert f(*p, WS, 3, 4, Hq, Hkv, 40, 6, 16, 128, None) == -2, (Hq, Hkv)
    for page in (1, 8, 48, 100, 512):
        assert f(*p, WS, 3, 4, 8, 2, 40, 6, page, 128, None) == -2, page
    assert f(*p, WS, 3, 4, 8, 2, 40, 1 << 23, 256, 128, None) == -2  # max_pages page = 2^31
    split = (1, 2, 4, 1, 40, 256, 16, 128)  # 16 splits: the workspace is required, and large enough
    need = _plan(MULTI_P, *split[:4], *split[5:])[1][2]
    assert need == 1 * 2 * 4 * 16 * 130 * 4
    assert f(*p[:7], None, 0, *split, None) == -1 and f(*p, need - 1, *split, None) == -1


def test_python_entries_ask_for_bfloat16_before_any_device_call(built):
    """fp16 (and fp32) tensors raise `values must be torch::kBFloat16` -- the dtype check comes first, so CPU tensors get there without a GPU -- and
    bf16 tensors get past it to the device check."""
    want = re.compile(r"^values must be torch::kBFloat16$")  # the text of host._TH_NAME, as fp16 raises torch::kHalf
    i32 = torch.int32
    ints = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32))
    for dt in (torch.float16, torch.float32):
        t = lambda *s: torch.zeros(*s, dtype=dt)  # noqa: E731
        with pytest.raises(RuntimeError) as e:
            built.fa2_prefill_paged_varlen_bf16(t(40, 8, 64), t(9, 2, 16, 64), t(9, 2, 16, 64), *ints, t(40, 8, 64))
        assert want.search(str(e.value)), e.value
        with pytest.raises(RuntimeError) as e:
            built.kv_append_paged_varlen_bf16(t(40, 2, 64), t(40, 2, 64), t(9, 2, 16, 64), t(9, 2, 16, 64), *ints)
        assert want.search(str(e.value)), e.value
        with pytest.raises(RuntimeError) as e:
            built.fa2_decode_paged_multi_bf16(t(2, 3, 8, 64), t(9, 2, 16, 64), t(9, 2, 16, 64), *ints[:2], t(2, 3, 8, 64))
        assert want.search(str(e.value)), e.value
    b = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)  # noqa: E731
    for one_fp16 in range(4):  # a single fp16 tensor among bf16 ones: q, k_pages, v_pages, out
        args = [b(40, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), b(40, 8, 64)]
        args[one_fp16] = args[one_fp16].half()
        with pytest.raises(RuntimeError) as e:
            built.fa2_prefill_paged_varlen_bf16(*args[:3], *ints, args[3])
        assert want.search(str(e.value)), (one_fp16, e.value)
    with pytest.raises(RuntimeError, match="no CPU path"):
        built.fa2_prefill_paged_varlen_bf16(b(40, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints, b(40, 8, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        built.kv_append_paged_varlen_bf16(b(40, 2, 64), b(40, 2, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints)
    with pytest.raises(RuntimeError, match="no CPU path"):
        built.fa2_decode_paged_multi_bf16(b(2, 3, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints[:2], b(2, 3, 8, 64))
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen_bf16: rope 'neox' not supported"):
        built.kv_append_paged_varlen_bf16(b(40, 2, 64), b(40, 2, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints, rope="neox")
    with pytest.raises(RuntimeError, match="values must be"):  # the fp16 entries keep refusing bf16
        built.fa2_prefill_paged_varlen(b(40, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints, b(40, 8, 64))


def _bodies(src, tmp_path):
    import kernel_resources as kres
    kernels, s = kres.report(os.path.join(CSRC, src), keep=str(tmp_path))
    text = open(s).read()
    out = []
    for k in kernels:
        body = text[text.index("\n" + k["name"] + ":"):]
        out.append((k, body[:body.index(".Lfunc_end")]))
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert not k["name"].endswith("_kernel") and "_kernelI" not in k["name"], k["name"]
        assert "_f16" not in body and "atomic" not in body, k["name"]  # no fp16 MFMA, no conversion through fp16
    return out


def test_prefill_kernels_run_both_products_on_the_bf16_matrix_pipe_with_the_fp16_siblings_registers(tmp_path):
    got = _bodies("flash_attn_prefill_paged_varlen_bf16.hip", tmp_path)
    assert len(got) == 2 and all("fa2_prefill_paged_varlen_bf16_mfma" in k["name"] for k, _ in got), [k["name"] for k, _ in got]
    for k, body in got:
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")})
        D = 128 if k["lds"] > 30000 else 64
        assert k["vgpr"] <= (222 if D == 128 else 155), k  # the fp16 siblings' registers
        assert 0 < 2 * k["lds"] <= LDS_PER_CU and k["vgpr"] <= 256, k  # two workgroups per CU, two waves per SIMD
        assert body.count("v_mfma_f32_16x16x32_bf16") == D // 2 and "ds_read_b64_tr_b16" in body and "global_load_dwordx4" in body, k["name"]
        assert "v_cvt_pk_bf16_f32" in body, k["name"]  # P and O: round to nearest even in hardware


def test_multi_kernels_and_the_bf16_combine(tmp_path):
    got = _bodies("flash_attn_decode_paged_multi_bf16.hip", tmp_path)
    stream = [(k, b) for k, b in got if "fa2_decode_paged_multi_bf16_mfma" in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_bf16_rows" in k["name"]]
    assert len(stream) == 8 and len(combine) == 2 and len(got) == 10, [k["name"] for k, _ in got]
    for k, body in stream:
        assert "v_mfma_f32_16x16x32_bf16" in body and "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]
        assert k["vgpr"] <= 512, k
    for k, body in combine:
        assert "v_cvt_pk_bf16_f32" in body and "global_store_short" in body and "v_mfma" not in body, k["name"]


def test_append_kernels_move_sixteen_bytes_and_round_once(tmp_path):
    got = _bodies("kv_append_paged_varlen_bf16.hip", tmp_path)
    assert len(got) == 6 and all("kv_append_paged_varlen_bf16_rows" in k["name"] for k, _ in got), [k["name"] for k, _ in got]
    for k, body in got:
        assert k["lds"] == 0, k
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, k["name"]
        assert "global_store_short" not in body and "global_store_dword " not in body and " nt" not in body, k["name"]  # whole pieces, plain stores
    assert sorted(body.count("v_cvt_pk_bf16_f32") for _, body in got) == [0, 0, 8, 8, 16, 16]  # none for a copy, one per rotated pair of outputs
