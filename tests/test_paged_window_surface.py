"""CPU: the sliding-window entries of the bf16 paged KV-cache path (include/cln_amd_ext.h: cln_fa2_prefill_paged_varlen_window_bf16,
cln_fa2_decode_paged_multi_window_bf16 with their plan / describe entries; csrc/*_window_bf16.{cuh,hip}, paged::multi_window_plan in
csrc/paged_entry.h) -- header, exports, the plan against its Python mirror (tests/paged_window_reference.py) and against the unwindowed plan, the
live splits of every length, every status code before any device access against the unwindowed sibling's, the describe texts, the Python errors,
and the kernels' resources. No GPU needed: hipcc cross-compiles."""
import ctypes
import itertools
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
import paged_decode_reference as pr  # noqa: E402
import paged_window_reference as wr  # noqa: E402

PREFILL, PREFILL_D = "cln_fa2_prefill_paged_varlen_window_bf16", "cln_fa2_prefill_paged_varlen_window_bf16_describe"
MULTI, MULTI_P, MULTI_D = ("cln_fa2_decode_paged_multi_window_bf16", "cln_fa2_decode_paged_multi_window_bf16_plan",
                           "cln_fa2_decode_paged_multi_window_bf16_describe")
NAMES = (PREFILL, PREFILL_D, MULTI, MULTI_P, MULTI_D)
SIBLING = {n: n.replace("_window_bf16", "_bf16") for n in NAMES}
LDS_PER_CU = 160 * 1024
INT_MAX = wr.INT_MAX


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_five_prototypes(tmp_path, lang, cc):
    """The sibling's argument lists with `int window` behind D."""
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a1)(const void*, const void*, const void*, const int*, const int*, const int*, void*, float*, int, int, int, int, int,"
                   " int, int, int, int, void*) = %s;\n"
                   "int (*t1)(int, int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int (*a3)(const void*, const void*, const void*, const int*, const int*, void*, float*, void*, long long, int, int, int, int,"
                   " int, int, int, int, int, void*) = %s;\n"
                   "int (*p3)(int, int, int, int, int, int, int, int, int*, int*, long long*) = %s;\n"
                   "int (*t3)(int, int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int main(void) { return a1 && t1 && a3 && p3 && t3 ? 0 : 1; }\n" % NAMES)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _fn(name, argtypes):
    fn = getattr(_lib(), name)
    fn.argtypes, fn.restype = argtypes, ctypes.c_int
    return fn


def _prefill(window):
    return _fn(PREFILL if window else SIBLING[PREFILL], [ctypes.c_void_p] * 8 + [ctypes.c_int] * (8 + window) + [ctypes.c_void_p])


def _multi(window):
    return _fn(MULTI if window else SIBLING[MULTI], [ctypes.c_void_p] * 8 + [ctypes.c_longlong] + [ctypes.c_int] * (8 + window) + [ctypes.c_void_p])


def _plan(name, *dims):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_void_p] * 3)
    s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    rc = fn(*dims, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
    return rc, (s.value, c.value, w.value)


def _describe(name, *dims):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(2048)
    rc = fn(*dims, buf, 2048)
    return rc, buf.value.decode()


def test_library_header_and_package_hold_the_entries(built):
    lib, hdr = _lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_prefill_paged_varlen_window_bf16", "fa2_decode_paged_multi_window_bf16", "fa2_decode_paged_multi_window_bf16_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    for n in ("describe_prefill_paged_varlen_window_bf16", "describe_decode_paged_multi_window_bf16"):
        assert hasattr(built.manifest, n), n
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:  # none of the new names is a manifest name
        assert n not in names and n.replace("cln_", "") not in names


WINDOWS = (1, 17, 127, 128, 129, 1000, 1024, 4096, 1 << 20, INT_MAX)


def test_plan_is_its_mirror_covers_the_span_and_is_the_unwindowed_plan_for_a_window_past_the_cache(built):
    n = split = 0
    for B, T, (Hq, Hkv), (mp, page), D, W in itertools.product((1, 2, 7, 64, 4096), (1, 3, 8), ((1, 1), (8, 2), (32, 8), (8, 1)),
                                                               ((1, 16), (19, 16), (256, 16), (1024, 16), (16, 256), (64, 256), (4, 64)),
                                                               (64, 128), WINDOWS):
        rc, got = _plan(MULTI_P, B, T, Hq, Hkv, mp, page, D, W)
        assert rc == 0, (B, T, Hq, Hkv, mp, page, D, W)
        assert got == wr.plan(B, T, Hq, Hkv, mp, page, D, W) == built.fa2_decode_paged_multi_window_bf16_plan(B, T, Hq, Hkv, mp, page, D, W)
        S, C, ws = got
        span = wr.span(T, mp, page, W)
        assert S * C >= span > (S - 1) * C and C % wr.unit(page) == 0 and span <= mp * page
        if W >= mp * page:  # exactly the unwindowed plan
            assert (rc, got) == _plan(SIBLING[MULTI_P], B, T, Hq, Hkv, mp, page, D), (B, T, Hq, Hkv, mp, page, D, W)
        n += 1
        split += S > 1
    assert n > 5000 and split > 500


def test_plan_splits_the_window_not_the_cache(built):
    """B = 1, T = 1, max_pages page = 16384, W = 1024: the span of 1152 keys is split, where the unwindowed plan's chunk of 384 keys would leave all
    but four of its 43 splits without a key."""
    for Hkv in (1, 8):
        S, C, _ = built.fa2_decode_paged_multi_window_bf16_plan(1, 1, 4 * Hkv, Hkv, 1024, 16, 128, 1024)
        span = wr.span(1, 1024, 16, 1024)
        assert span == 1152 and S > 1 and span <= S * C < 2 * span, (S, C)
        assert wr.live_splits(16384, 1, 1024, 16, C) == S  # every split of a long sequence holds keys
    fn = _fn(MULTI_P, [ctypes.c_int] * 8 + [ctypes.c_void_p] * 3)
    assert fn(1, 1, 8, 2, 256, 16, 128, 100, None, None, None) == 0  # every out-parameter may be null


@pytest.mark.parametrize("W,T,page,mp", [(1, 1, 16, 64), (33, 4, 16, 64), (128, 8, 16, 64), (129, 8, 256, 8), (1000, 4, 16, 256), (1000, 8, 256, 16),
                                         (4096, 1, 64, 64), (5000, 8, 16, 256)])
def test_live_splits_of_every_length_fit_the_plan(built, W, T, page, mp):
    """Brute force over len in [0, Nmax]: base is a multiple of U at or below the first query's lower edge, and ceil((len - base) / C) <= S."""
    Nmax, U = mp * page, wr.unit(page)
    for (B, Hkv) in ((1, 1), (64, 8)):
        S, C, _ = built.fa2_decode_paged_multi_window_bf16_plan(B, T, Hkv, Hkv, mp, page, 128, W)
        worst = 0
        for n in range(Nmax + 1):
            base = wr.base(n, T, W, U)
            assert base % U == 0 and base <= wr.lo_min(n, T, W) < base + U
            worst = max(worst, wr.live_splits(n, T, W, page, C))
        assert 1 <= worst <= S, (worst, S, C)


def _shape_errors():
    """(B, T | total_q, Hq, Hkv, max_pages, page, D) that the unwindowed entries refuse, and some they take."""
    return [(0, 2, 8, 8, 4, 16, 64), (1, 0, 8, 8, 4, 16, 64), (1, 2, 0, 8, 4, 16, 64), (1, 2, 8, 0, 4, 16, 64), (1, 2, 8, 8, 0, 16, 64),
            (1, 2, 8, 8, 4, 0, 64), (1, 2, 8, 8, 4, 16, 0), (-2, 2, 8, 8, 4, 16, 64), (1, 2, 8, 3, 4, 16, 64), (1, 2, 8, 8, 4, 16, 96),
            (1, 2, 8, 8, 4, 16, 32), (1, 2, 3, 1, 4, 16, 64), (1, 2, 16, 1, 4, 16, 64), (1, 2, 8, 8, 4, 48, 64), (1, 2, 8, 8, 4, 8, 64),
            (1, 2, 8, 8, 4, 512, 64), (1, 2, 8, 8, 1 << 23, 256, 64), (1, 1 << 28, 8, 1, 4, 16, 64), (1 << 24, 1, 8, 8, 4, 16, 64),
            (1, 9, 8, 8, 4, 16, 64), (1, 170, 8, 8, 4, 16, 64), (1, 2, 8, 8, 4, 16, 64), (3, 8, 8, 2, 40, 16, 128), (1, 1, 8, 8, 1024, 16, 128)]


def test_describe_and_plan_statuses_are_the_unwindowed_siblings_and_a_window_below_one_is_minus_one(built):
    ok = 0
    for dims in _shape_errors():
        for W in (1, 200, INT_MAX):
            for name in (PREFILL_D, MULTI_D):
                a, b = _describe(name, *dims, W)[0], _describe(SIBLING[name], *dims)[0]
                assert min(a, 0) == min(b, 0), (name, dims, W, a, b)
                ok += a > 0
            assert _plan(MULTI_P, *dims, W)[0] == _plan(SIBLING[MULTI_P], *dims)[0], (dims, W)
    assert ok
    good = (3, 8, 8, 2, 40, 16, 128)
    for W in (0, -1, -INT_MAX - 1):
        assert _describe(PREFILL_D, *good, W)[0] == _describe(MULTI_D, *good, W)[0] == -1
        rc, out = _plan(MULTI_P, *good, W)
        assert rc == -1 and out == (-7, -7, -7)  # a refusal leaves the out-parameters alone
    with pytest.raises(ValueError):
        built.manifest.describe_prefill_paged_varlen_window_bf16(*good, 0)
    with pytest.raises(ValueError):
        built.manifest.describe_decode_paged_multi_window_bf16(*good, 0)
    with pytest.raises(ValueError):
        built.manifest.describe_decode_paged_multi_window_bf16(1, 9, 8, 8, 4, 16, 64, 5)


# q, k_pages, v_pages, block_table, seqlens, cu_q, o, lse: never dereferenced, every call below fails its checks first
PTR = [0x10000 * (i + 1) for i in range(8)]
DIMS = (3, 170, 8, 2, 40, 6, 16, 128)  # B, total_q, Hq, Hkv, P, max_pages, page, D
BAD_D = DIMS[:7] + (96,)


def test_prefill_statuses_are_the_siblings_before_any_device_access(built):
    f, g = _prefill(1), _prefill(0)
    p = list(PTR)

    def both(ptrs, dims, want):
        a, b = f(*ptrs, *dims, 5, None), g(*ptrs, *dims, None)
        assert a == b == want, (ptrs, dims, a, b)
    both(p, BAD_D, -2)
    both(p[:7] + [None], BAD_D, -2)
    for i in range(7):  # a null required pointer
        a = list(p)
        a[i] = None
        both(a, DIMS, -1)
    for i, off in ((0, 8), (1, 8), (2, 8), (6, 8), (3, 2), (4, 2), (5, 2), (7, 2)):  # alignment: 16 bytes for the tensors, 4 for the int32 arrays and lse
        a = list(p)
        a[i] = p[i] + off
        both(a, DIMS, -1)
    for out in (6, 7):  # an output equal to an input or to the other output
        for src in range(8):
            if src != out:
                a = list(p)
                a[out] = p[src]
                both(a, DIMS, -1)
    for i in range(8):  # each dimension non-positive
        d = list(DIMS)
        d[i] = 0
        both(p, d, -1)
    both(p, (3, 170, 8, 3, 40, 6, 16, 128), -1)  # Hq % Hkv
    for d in ((3, 170, 6, 2, 40, 6, 16, 128), (3, 170, 8, 2, 40, 6, 48, 128), (3, 170, 8, 2, 40, 1 << 23, 256, 128), (1, 1 << 28, 8, 1, 40, 6, 16, 128),
              (1 << 24, 1, 8, 8, 40, 6, 16, 64)):
        both(p, d, -2)
    for W in (0, -1, -INT_MAX - 1):  # the window alone is wrong: -1, and behind the shape: an unsupported D stays -2
        assert f(*p, *DIMS, W, None) == -1 and f(*p, *BAD_D, W, None) == -2


MPTR = [0x10000 * (i + 1) for i in range(8)]  # q, k_pages, v_pages, block_table, seqlens, o, lse, workspace
MDIMS = (3, 4, 8, 2, 40, 6, 16, 128)          # B, T, Hq, Hkv, P, max_pages, page, D: one split, no workspace needed
MBAD_D = MDIMS[:7] + (96,)
WS = 1 << 30


def test_multi_statuses_are_the_siblings_before_any_device_access(built):
    f, g = _multi(1), _multi(0)
    p = list(MPTR)

    def both(ptrs, ws, dims, want):
        a, b = f(*ptrs, ws, *dims, 5, None), g(*ptrs, ws, *dims, None)
        assert a == b == want, (ptrs, dims, a, b)
    both(p, WS, MBAD_D, -2)
    both(p[:6] + [None, None], 0, MBAD_D, -2)
    for i in range(6):
        a = list(p)
        a[i] = None
        both(a, WS, MDIMS, -1)
    for i, off in ((0, 8), (1, 8), (2, 8), (5, 8), (6, 8), (7, 8), (3, 2), (4, 2)):
        a = list(p)
        a[i] = p[i] + off
        both(a, WS, MDIMS, -1)
    for out in (5, 6, 7):
        for src in range(8):
            if src != out:
                a = list(p)
                a[out] = p[src]
                both(a, WS, MDIMS, -1)
    for i in range(8):
        d = list(MDIMS)
        d[i] = 0
        both(p, WS, d, -1)
    both(p, WS, (3, 4, 8, 3, 40, 6, 16, 128), -1)
    for d in ((3, 9, 8, 2, 40, 6, 16, 128), (3, 4, 6, 2, 40, 6, 16, 128), (3, 4, 8, 2, 40, 6, 48, 128), (3, 4, 8, 2, 40, 1 << 23, 256, 128)):
        both(p, WS, d, -2)
    for W in (0, -1, -INT_MAX - 1):
        assert f(*p, WS, *MDIMS, W, None) == -1 and f(*p, WS, *MBAD_D, W, None) == -2
    split = (1, 2, 4, 1, 40, 256, 16, 128)  # max_pages page = 4096 and W = 1000: 3 splits, the workspace is required, and large enough
    rc, (S, C, need) = _plan(MULTI_P, *split[:4], *split[5:], 1000)
    assert rc == 0 and (S, C) == (3, 384) and need == 1 * 2 * 4 * 3 * 130 * 4
    assert f(*p[:7], None, 0, *split, 1000, None) == -1 and f(*p, need - 1, *split, 1000, None) == -1


def test_describe_texts_match_the_python_mirrors(built):
    m = built.manifest
    for D, G, page, W in itertools.product((64, 128), pr.GROUPS, pr.PAGES, (1, 200, 1024, INT_MAX)):
        for (B, tq, Hkv, mp) in ((1, 1, 1, 1), (5, 204, 1, 32), (65, 2112, 8, 300)):
            Hq = Hkv * G
            rc, text = _describe(PREFILL_D, B, tq, Hq, Hkv, mp, page, D, W)
            assert rc == len(text) > 0, (rc, text)
            assert text == m.describe_prefill_paged_varlen_window_bf16(B, tq, Hq, Hkv, mp, page, D, W)
            assert text == wr.describe_prefill_text(B, tq, Hq, Hkv, mp, page, D, W)
            assert text.startswith("fa2_prefill_paged_varlen_window_bf16_mfma<D=%d,G=%d> B=%d" % (D, G, B)) and " W=%d:" % W in text
            assert "a span of at most %d keys" % min(W + 128 // G + 128, mp * page) in text and "S=1" in text
        for (B, T, Hkv, mp) in ((1, 1, 1, 256), (7, 3, 2, 19), (64, 8, 8, 300), (1, 8, 1, 4096)):
            Hq = Hkv * G
            rc, text = _describe(MULTI_D, B, T, Hq, Hkv, mp, page, D, W)
            assert rc == len(text) > 0, (rc, text)
            assert text == m.describe_decode_paged_multi_window_bf16(B, T, Hq, Hkv, mp, page, D, W) == wr.describe_multi_text(B, T, Hq, Hkv, mp, page, D, W)
            S, C, _ = wr.plan(B, T, Hq, Hkv, mp, page, D, W)
            assert text.startswith("fa2_decode_paged_multi_window_bf16_mfma<D=%d,MT=%d> T=%d G=%d W=%d span=%d S=%d C=%d "
                                   % (D, -(-T * G // 16), T, G, W, wr.span(T, mp, page, W), S, C))
            assert ("fa2_decode_combine_window_bf16_rows<D=%d>" % D in text) == (S > 1)
    for name, dims in ((PREFILL_D, (1, 1, 8, 2, 4, 16, 64, 9)), (MULTI_D, (1, 1, 8, 2, 4, 16, 64, 9))):
        rc, text = _describe(name, *dims)
        f = getattr(_lib(), name)
        small = ctypes.create_string_buffer(b"\xff" * 24, 24)
        assert f(*dims, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
        assert f(*dims, None, 16) == -1 and f(*dims, small, 0) == -1


def test_python_entries_refuse_a_window_below_one_and_other_dtypes_before_any_device_call(built):
    i32 = torch.int32
    ints = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32))
    b = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)  # noqa: E731
    for W in (0, -3):
        with pytest.raises(RuntimeError) as e:
            built.fa2_prefill_paged_varlen_window_bf16(b(40, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints, W, b(40, 8, 64))
        assert str(e.value) == "fa2_prefill_paged_varlen_window_bf16: window %d not supported (>= 1)" % W
        with pytest.raises(RuntimeError) as e:
            built.fa2_decode_paged_multi_window_bf16(b(2, 3, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints[:2], W, b(2, 3, 8, 64))
        assert str(e.value) == "fa2_decode_paged_multi_window_bf16: window %d not supported (>= 1)" % W
        with pytest.raises(RuntimeError) as e:
            built.fa2_decode_paged_multi_window_bf16_plan(2, 3, 8, 2, 4, 16, 64, W)
        assert str(e.value) == "fa2_decode_paged_multi_window_bf16: window %d not supported (>= 1)" % W
    want = re.compile(r"^values must be torch::kBFloat16$")
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)  # noqa: E731
    with pytest.raises(RuntimeError) as e:
        built.fa2_prefill_paged_varlen_window_bf16(h(40, 8, 64), h(9, 2, 16, 64), h(9, 2, 16, 64), *ints, 5, h(40, 8, 64))
    assert want.search(str(e.value)), e.value
    with pytest.raises(RuntimeError) as e:
        built.fa2_decode_paged_multi_window_bf16(h(2, 3, 8, 64), h(9, 2, 16, 64), h(9, 2, 16, 64), *ints[:2], 5, h(2, 3, 8, 64))
    assert want.search(str(e.value)), e.value
    with pytest.raises(RuntimeError, match="no CPU path"):
        built.fa2_prefill_paged_varlen_window_bf16(b(40, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints, 5, b(40, 8, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        built.fa2_decode_paged_multi_window_bf16(b(2, 3, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints[:2], 5, b(2, 3, 8, 64))
    with pytest.raises(RuntimeError, match=r"fa2_decode_paged_multi_window_bf16: T 9 not supported"):
        built.fa2_decode_paged_multi_window_bf16_plan(1, 9, 8, 2, 4, 16, 64, 5)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_window_bf16: headdim 96"):
        built.fa2_decode_paged_multi_window_bf16_plan(1, 1, 8, 2, 4, 16, 96, 5)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_window_bf16: 8 query heads are no multiple of 3 KV heads"):
        built.fa2_decode_paged_multi_window_bf16_plan(1, 1, 8, 3, 4, 16, 64, 5)


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


def test_prefill_kernels_keep_two_workgroups_per_cu_without_spill_or_scratch(tmp_path):
    got = _bodies("flash_attn_prefill_paged_varlen_window_bf16.hip", tmp_path)
    assert len(got) == 2 and all("fa2_prefill_paged_varlen_window_bf16_mfma" in k["name"] for k, _ in got), [k["name"] for k, _ in got]
    for k, body in got:
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")})
        D = 128 if k["lds"] > 30000 else 64
        assert 0 < 2 * k["lds"] <= LDS_PER_CU and k["vgpr"] <= 256, k  # two workgroups per CU, two waves per SIMD
        assert body.count("v_mfma_f32_16x16x32_bf16") == D // 2 and "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]


def test_multi_kernels_and_the_window_combine_without_spill_or_scratch(tmp_path):
    got = _bodies("flash_attn_decode_paged_multi_window_bf16.hip", tmp_path)
    stream = [(k, b) for k, b in got if "fa2_decode_paged_multi_window_bf16_mfma" in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_window_bf16_rows" in k["name"]]
    assert len(stream) == 8 and len(combine) == 2 and len(got) == 10, [k["name"] for k, _ in got]
    for k, body in stream:
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")})
        assert "v_mfma_f32_16x16x32_bf16" in body and "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]
        assert k["vgpr"] <= 512, k
    for k, body in combine:
        assert "v_cvt_pk_bf16_f32" in body and "global_store_short" in body and "v_mfma" not in body, k["name"]
