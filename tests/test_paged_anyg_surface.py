"""CPU: the paged bf16 attention entries for any query-group size G = Hq / Hkv in 1 ... 16 (include/cln_amd_ext.h:
cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16[_fp8], cln_fa2_decode_paged_multi_window_sink_anyg_bf16[_fp8] with their plan / describe
entries; csrc/*_anyg_*.{cuh,hip}) -- header and exports, every status code before any device access against the power-of-two
siblings' and then those of G, T G and an optional `sinks`, the plan against the siblings' and against fa2d::split_plan evaluated in Python, the
describe texts, the Python errors, the sensitivity of the GPU cases to the three wrong row maps they exist for, and the kernels' resources and
instructions against the siblings'. No GPU needed: hipcc cross-compiles."""
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
sys.path.insert(0, os.path.join(ROOT, "cuda-learn-notes_amd", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_anyg_cases as ac  # noqa: E402
import paged_bf16_fp8_reference as fr  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import paged_window_reference as wr  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of a code object)

PRE, PRE8 = "cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16", "cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8"
DEC, DEC8 = "cln_fa2_decode_paged_multi_window_sink_anyg_bf16", "cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8"
NAMES = (PRE, PRE + "_describe", DEC, DEC + "_plan", DEC + "_describe", PRE8, PRE8 + "_describe", DEC8, DEC8 + "_plan", DEC8 + "_describe")
SIB = lambda n: n.replace("_anyg_", "_")  # noqa: E731
INT_MAX = sr.INT_MAX
BF = torch.bfloat16
INT9 = [ctypes.c_int] * 9
_fn, _plan, _describe = fs._fn, fs._plan, fs._describe


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_ten_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    pre = "const void*, const void*, const void*, const int*, const int*, const int*, %sconst float*, void*, float*, " + "int, " * 9 + "void*"
    dec = ("const void*, const void*, const void*, const int*, const int*, %sconst float*, void*, float*, void*, long long, " + "int, " * 9
           + "void*")
    text, plan = "int, int, int, int, int, int, int, int, char*, int", "int, int, int, int, int, int, int, int, int*, int*, long long*"
    protos = (pre % "", text, dec % "", plan, text, pre % "const float*, const float*, ", text, dec % "const float*, const float*, ", plan, text)
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip(protos, NAMES)))
                   + "int main(void) { return f0 && f9 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_and_package_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in (PRE, DEC, DEC + "_plan", PRE8, DEC8, DEC8 + "_plan"):
        assert hasattr(built, n[4:]) and hasattr(host, n[4:]), n
    for n in (PRE, DEC, PRE8, DEC8):
        assert hasattr(built.manifest, "describe_" + n[len("cln_fa2_"):]), n
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:  # none of the new names is a manifest name
        assert n not in names and n.replace("cln_", "") not in names


# ---------------------------------------------------------------------------------------------------- plan

def test_plan_is_the_siblings_for_powers_of_two_status_included(built):
    """The sibling surface test's grid with G in {1, 2, 4, 8}: status and plan equal, for both new plans."""
    n = split = 0
    for B, T, (G, Hkv), (mp, page), D, W in itertools.product((1, 5, 64), (1, 3, 8), ((1, 1), (8, 1), (8, 8), (2, 3), (4, 2)),
                                                              ((19, 16), (256, 16), (1024, 16), (64, 256)), (64, 128),
                                                              (1, 33, 128, 1000, 4096, 1 << 20, INT_MAX)):
        Hq = G * Hkv
        want = _plan(SIB(DEC) + "_plan", B, T, Hq, Hkv, mp, page, D, W)
        assert want[0] == 0
        for name in (DEC, DEC8):
            assert _plan(name + "_plan", B, T, Hq, Hkv, mp, page, D, W) == want, (name, B, T, Hq, Hkv, mp, page, D, W)
        assert built.fa2_decode_paged_multi_window_sink_anyg_bf16_plan(B, T, Hq, Hkv, mp, page, D, W) == want[1]
        n += 1
        split += want[1][0] > 1
    assert n > 1000 and split > 100
    # refusals: the siblings' status for the same arguments (none of these has a G the siblings refuse and the new entries take)
    for dims in ((0, 2, 8, 8, 4, 16, 64), (1, 9, 8, 8, 4, 16, 64), (1, 2, 8, 3, 4, 16, 64), (1, 2, 8, 8, 4, 16, 96), (1, 2, 8, 8, 4, 48, 64),
                 (1, 2, 0, 8, 4, 16, 64), (1, 2, 8, 0, 4, 16, 64), (1, 2, 8, 8, 0, 16, 64), (1, 2, 8, 8, 1 << 23, 256, 64), (1, 2, 17, 1, 4, 16, 64)):
        for W in (5, 0):
            for name in (DEC, DEC8):
                assert _plan(name + "_plan", *dims, W) == _plan(SIB(name) + "_plan", *dims, W), (name, dims, W)
                for d in (name + "_describe", name.replace("decode_paged_multi", "prefill_paged_varlen") + "_describe"):
                    a, b = _describe(d, *dims, W)[0], _describe(SIB(d), *dims, W)[0]
                    assert min(a, 0) == min(b, 0), (d, dims, W, a, b)


def test_plan_for_the_other_groups_is_split_plan_in_python(built):
    """G in {3, 5, 7, 12, 16}: the plan is fa2d::split_plan on B Hkv, B T Hq, the window entry's span and unit -- paged_window_reference.plan, which
    never looks at G."""
    n = split = 0
    for B, (T, G), Hkv, (mp, page), D, W in itertools.product((1, 5, 64), ((1, 3), (3, 5), (8, 5), (8, 7), (1, 7), (5, 12), (4, 16), (1, 16)),
                                                              (1, 2, 8), ((19, 16), (256, 16), (1024, 16), (64, 256)), (64, 128),
                                                              (1, 33, 1000, 4096, INT_MAX)):
        Hq = G * Hkv
        want = wr.plan(B, T, Hq, Hkv, mp, page, D, W)
        for name in (DEC, DEC8):
            assert _plan(name + "_plan", B, T, Hq, Hkv, mp, page, D, W) == (0, want), (name, B, T, Hq, Hkv, mp, page, D, W)
            assert _plan(SIB(name) + "_plan", B, T, Hq, Hkv, mp, page, D, W)[0] == -2  # and the siblings keep refusing
        assert built.fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan(B, T, Hq, Hkv, mp, page, D, None if W == INT_MAX else W) == want
        n += 1
        split += want[0] > 1
    assert n > 1000 and split > 100


# ---------------------------------------------------------------------------------------------------- status codes
# Never dereferenced: every call below fails its checks first.

SINKS, KS, VS = 0x10000 * 20, 0x10000 * 21, 0x10000 * 22


def _statuses(f, g, fp8, n_in, n_out, tail, dims, bad_d, sib_optional):
    """f: the new entry, g: its power-of-two sibling, the same argument list. The sibling's status for the same arguments, argument by argument;
    then sinks: NULL legal, misaligned or an output -1."""
    p = [0x10000 * (i + 1) for i in range(n_in + n_out)]
    sc = (KS, VS) if fp8 else ()

    def call(fn, ptrs, d, sinks=SINKS, W=5):
        return fn(*ptrs[:n_in], *sc, sinks, *ptrs[n_in:], *tail, *d, W, None)

    def both(ptrs, d, want, W=5):
        a, b = call(f, ptrs, d, W=W), call(g, ptrs, d, W=W)
        assert a == b == want, (ptrs, d, W, a, b)
        assert call(f, ptrs, d, None, W=W) == want  # ... and without sinks
        if sib_optional:
            assert call(g, ptrs, d, None, W=W) == want
    both(p, bad_d, -2)
    for i in range(n_in + 1):  # a null required pointer (the first output too)
        a = list(p)
        a[i] = None
        both(a, dims, -1)
    for i in range(n_in + n_out):
        a = list(p)
        a[i] = p[i] + (2 if 3 <= i < n_in else 8 if i < n_in + 1 else 2)
        both(a, dims, -1)
    for out in range(n_in, n_in + n_out):  # an output equal to an input or to another output
        for src in range(n_in + n_out):
            if src != out:
                a = list(p)
                a[out] = p[src]
                both(a, dims, -1)
    for i in range(8):  # each dimension non-positive
        d = list(dims)
        d[i] = 0
        both(p, d, -1)
    for W in (0, -1, -INT_MAX - 1):  # window <= 0: -1, behind the shape
        both(p, dims, -1, W)
        both(p, bad_d, -2, W)
    for d in (dims, bad_d):
        for bad in (SINKS + 1, SINKS + 2) + tuple(p[n_in:]):  # sinks: misaligned, or an output
            assert call(f, p, d, bad) == -1, (bad, d)
    assert call(f, p, bad_d, SINKS + 4) == -2  # 4-byte alignment is enough: the shape is looked at
    assert call(f, p, bad_d, None) == -2
    return p, call


def _with(dims, **kw):
    """dims = (B, T | total_q, Hq, Hkv, P, max_pages, page, D) with some replaced"""
    keys = ("B", "T", "Hq", "Hkv", "P", "mp", "page", "D")
    return tuple(kw.get(k, v) for k, v in zip(keys, dims))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_prefill_statuses_are_the_siblings_then_those_of_the_group_size(built, fp8):
    name = PRE8 if fp8 else PRE
    args = [ctypes.c_void_p] * (11 if fp8 else 9) + INT9 + [ctypes.c_void_p]
    f, g = _fn(name, args), _fn(SIB(name), args)
    dims = (3, 170, 8, 2, 40, 6, 16, 128)  # B, total_q, Hq, Hkv, P, max_pages, page, D
    p, call = _statuses(f, g, fp8, 6, 2, (), dims, dims[:7] + (96,), fp8)
    # a launch would follow status 0, so only refusals are called: the shape is read off a window of 0, which is -1 behind a good shape
    for G, Hkv in ((3, 2), (5, 8), (6, 2), (7, 4), (12, 8), (16, 1), (16, 8), (1, 1), (8, 8)):
        d = _with(dims, Hq=G * Hkv, Hkv=Hkv)
        assert call(f, p, d, W=0) == -1 and call(f, p, d, None, W=0) == -1, d
        assert call(f, p, _with(d, D=96), W=0) == -2 and call(f, p, _with(d, page=48), W=0) == -2
        if G not in (1, 2, 4, 8):
            assert call(g, p, d, W=0) == -2, d  # the sibling refuses the group size
    for Hq, Hkv in ((17, 1), (34, 2), (256, 8), (1 << 20, 1)):  # G > 16
        assert call(f, p, _with(dims, Hq=Hq, Hkv=Hkv)) == -2 and call(f, p, _with(dims, Hq=Hq, Hkv=Hkv), W=0) == -2
    for Hq, Hkv in ((8, 3), (7, 2), (1, 2), (17, 16)):  # Hq % Hkv
        assert call(f, p, _with(dims, Hq=Hq, Hkv=Hkv)) == -1
    assert call(f, p, _with(dims, mp=1 << 23, page=256), W=0) == -2
    # the rows total_q G past an int: -2 for G = 3 at total_q = 2^30, a window of 0 is seen at total_q = 2^29
    assert call(f, p, _with(dims, T=1 << 30, Hq=3, Hkv=1), W=0) == -2 and call(f, p, _with(dims, T=1 << 29, Hq=3, Hkv=1), W=0) == -1
    # ... and for G = 7 the grid ends first: Hkv (total_q G / 128 + B) workgroups of 256 threads below 2^32 threads, 2^24 - 1 slots
    top = ((1 << 24) - 1 - 3) * 128 // 7
    assert call(f, p, _with(dims, T=(1 << 31) // 7 + 1, Hq=7, Hkv=1), W=0) == -2 and call(f, p, _with(dims, T=top + 19, Hq=7, Hkv=1), W=0) == -2
    assert call(f, p, _with(dims, T=top, Hq=7, Hkv=1), W=0) == -1  # R = 2147483135 rows: the kernel's r / G is an unsigned division, exact there


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_statuses_are_the_siblings_then_those_of_the_group_size_and_the_rows(built, fp8):
    name = DEC8 if fp8 else DEC
    args = [ctypes.c_void_p] * (11 if fp8 else 9) + [ctypes.c_longlong] + INT9 + [ctypes.c_void_p]
    f, g = _fn(name, args), _fn(SIB(name), args)
    dims = (3, 4, 8, 2, 40, 6, 16, 128)  # B, T, Hq, Hkv, P, max_pages, page, D: one split, no workspace needed
    p, call = _statuses(f, g, fp8, 5, 3, (1 << 30,), dims, dims[:7] + (96,), fp8)
    for T, G in ((1, 3), (3, 5), (8, 6), (8, 7), (5, 12), (4, 16), (1, 16), (8, 8), (4, 13)):  # T <= 8 and T G <= 64
        d = _with(dims, T=T, Hq=G * 2)
        assert call(f, p, d, W=0) == -1 and call(f, p, d, None, W=0) == -1, d
        assert _plan(name + "_plan", *d[:4], *d[5:], 5)[0] == 0
    for T, G in ((5, 13), (9, 1), (9, 7), (8, 9), (5, 16), (6, 12), (4, 17), (1, 17)):  # T G = 65, T = 9, ..., G = 17: -2, window or not
        d = _with(dims, T=T, Hq=G * 2)
        assert call(f, p, d) == -2 and call(f, p, d, W=0) == -2 and call(f, p, d, None) == -2, d
        assert _plan(name + "_plan", *d[:4], *d[5:], 5)[0] == -2
    for Hq, Hkv in ((8, 3), (7, 2)):
        assert call(f, p, _with(dims, Hq=Hq, Hkv=Hkv)) == -1 and _plan(name + "_plan", 3, 4, Hq, Hkv, 6, 16, 128, 5)[0] == -1
    assert _plan(name + "_plan", 3, 4, 10, 2, 6, 16, 128, 0)[0] == -1 and _plan(name + "_plan", 3, 4, 10, 2, 6, 16, 128, -5)[0] == -1
    split = (1, 3, 5, 1, 40, 256, 16, 128)  # max_pages page = 4096 and W = 1000: the plan splits, the workspace is required, and large enough
    rc, (S, C, need) = _plan(name + "_plan", *split[:4], *split[5:], 1000)
    assert rc == 0 and S > 1 and (S, C, need) == wr.plan(*split[:4], *split[5:], 1000)
    q = [0x10000 * (i + 1) for i in range(8)]
    sc = (KS, VS) if fp8 else ()
    for sinks in (SINKS, None):
        assert f(*q[:5], *sc, sinks, *q[5:7], None, 0, *split, 1000, None) == -1
        assert f(*q[:5], *sc, sinks, *q[5:], need - 1, *split, 1000, None) == -1


# ---------------------------------------------------------------------------------------------------- describe, Python errors

DIV = "(t, g) = (r / G, r mod G) by division outside the key loop, any G in 1 ... 16"
NONE = "(fp32, natural log, unscaled; none when sinks is NULL"


def _swap(text, pairs):
    for a, b in pairs:
        assert text.count(a) == 1, (a, text)
        text = text.replace(a, b)
    return text


def prefill_text(fp8, B, tq, Hq, Hkv, mp, page, D, W):
    """The sibling's text (paged_sink_reference / paged_bf16_fp8_reference, which hold G as a number) with the any-G kernel's name, G outside the
    template arguments, the division, and for the bf16 entry the optional sinks."""
    G = Hq // Hkv
    mod = fr if fp8 else sr
    kern = "fa2_prefill_paged_varlen_window_sink_bf16%s_mfma" % ("_fp8" if fp8 else "")
    pairs = [("%s<D=%d,G=%d> B=" % (kern, D, G), "%s<D=%d> G=%d B=" % (kern.replace("_sink_", "_sink_anyg_"), D, G)),
             ("query rows t G + g of its sequence, 32 rows", "query rows t G + g of its sequence, %s, 32 rows" % DIV)]
    if not fp8:
        pairs.append(("(fp32, natural log, unscaled)", NONE + ")"))
    # the span: the siblings count 128 / G tokens in a tile; where G does not divide 128 a tile starts inside a token and touches up to
    # floor((G + 126) / G) + 1 (tile_tokens below)
    reach = lambda tokens: min(W + tokens + 2 * wr.KEY_STEP, mp * page)  # noqa: E731
    pairs.append(("a span of at most %d keys" % reach(wr.ROW_TILE // G), "a span of at most %d keys" % reach(tile_tokens(G))))
    return _swap(mod.describe_prefill_text(B, tq, Hq, Hkv, mp, page, D, W), pairs)


def tile_tokens(G):
    """The tokens that 128 consecutive rows starting at a multiple of 128 touch at most, by counting."""
    return max(len({r // G for r in range(row0, row0 + 128)}) for row0 in range(0, 128 * G, 128))


def decode_text(fp8, B, T, Hq, Hkv, mp, page, D, W):
    G = Hq // Hkv
    mod = fr if fp8 else sr
    tiles = -(-T * G // 16)
    kern = "fa2_decode_paged_multi_window_sink_bf16%s_mfma<" % ("_fp8" if fp8 else "")
    pairs = [(kern, kern.replace("_sink_", "_sink_anyg_")),
             ("(T x G, %d tiles of 16)" % tiles, "(T x G, %d tiles of 16; %s with T G <= 64)" % (tiles, DIV))]
    if not fp8:
        split = wr.plan(B, T, Hq, Hkv, mp, page, D, W)[0] > 1
        pairs.append(("(fp32, natural log, unscaled)", NONE + (": fa2_decode_combine_window_bf16_rows<D=%d> then)" % D if split else ")")))
    return _swap(mod.describe_multi_text(B, T, Hq, Hkv, mp, page, D, W), pairs)


def test_describe_texts_match_the_python_mirrors(built):
    m = built.manifest
    splits = set()
    for fp8, D, G, page, W in itertools.product((False, True), (64, 128), (1, 3, 4, 5, 6, 7, 8, 12, 16), (16, 64, 256), (1, 128, 1024, INT_MAX)):
        pre, dec = (PRE8, DEC8) if fp8 else (PRE, DEC)
        for (B, tq, Hkv, mp) in ((1, 1, 1, 1), (5, 204, 1, 32), (65, 2112, 8, 300)):
            Hq = Hkv * G
            rc, text = _describe(pre + "_describe", B, tq, Hq, Hkv, mp, page, D, W)
            assert rc == len(text) > 0, (rc, text)
            assert text == getattr(m, "describe_" + pre[len("cln_fa2_"):])(B, tq, Hq, Hkv, mp, page, D, W)
            assert text == prefill_text(fp8, B, tq, Hq, Hkv, mp, page, D, W)
            assert " G=%d B=%d " % (G, B) in text and DIV in text and NONE in text and "_f16" not in text
        for (B, T, Hkv, mp) in ((1, 1, 1, 256), (7, 3, 2, 19), (64, 8, 8, 300), (1, 4, 1, 4096)):
            if T * G > 64:
                assert _describe(dec + "_describe", B, T, Hkv * G, Hkv, mp, page, D, W)[0] == -2
                continue
            Hq = Hkv * G
            rc, text = _describe(dec + "_describe", B, T, Hq, Hkv, mp, page, D, W)
            assert rc == len(text) > 0, (rc, text)
            assert text == getattr(m, "describe_" + dec[len("cln_fa2_"):])(B, T, Hq, Hkv, mp, page, D, W)
            assert text == decode_text(fp8, B, T, Hq, Hkv, mp, page, D, W)
            S = wr.plan(B, T, Hq, Hkv, mp, page, D, W)[0]
            splits.add(S > 1)
            assert "<D=%d,MT=%d> T=%d G=%d W=%d " % (D, -(-T * G // 16), T, G, W) in text and DIV + " with T G <= 64" in text
            assert ("fa2_decode_combine_window_sink_bf16_rows<D=%d>" % D in text) == (S > 1) and NONE in text
    assert splits == {False, True}
    assert [tile_tokens(G) for G in (1, 3, 7, 8, 12, 16)] == [128, 44, 20, 16, 12, 8]
    with pytest.raises(ValueError):
        m.describe_prefill_paged_varlen_window_sink_anyg_bf16(3, 8, 34, 2, 40, 16, 128, 5)
    with pytest.raises(ValueError):
        m.describe_decode_paged_multi_window_sink_anyg_bf16_fp8(1, 5, 13, 1, 4, 16, 64, 5)


def test_python_entries_raise_the_siblings_errors_and_forward_none(built, monkeypatch):
    from cuda_learn_notes_amd import host
    import fp8_kv_reference as f8
    i32 = torch.int32
    ints = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32))
    b = lambda *s: torch.zeros(*s, dtype=BF)  # noqa: E731
    p8 = lambda: torch.zeros(9, 2, 16, 64, dtype=torch.uint8).view(f8.F8)  # noqa: E731
    pb = lambda: b(9, 2, 16, 64)  # noqa: E731
    sc = torch.ones(2)
    Hq = 14

    def pre(W=5, sinks=None, q=None, kp=None, any_=True):
        fn = built.fa2_prefill_paged_varlen_window_sink_anyg_bf16 if any_ else built.fa2_prefill_paged_varlen_window_sink_bf16
        return fn(b(40, Hq, 64) if q is None else q, pb() if kp is None else kp, pb(), *ints, W, sinks, b(40, Hq, 64) if q is None else torch.zeros_like(q))

    def dec(W=5, sinks=None, q=None, kp=None, any_=True):
        fn = built.fa2_decode_paged_multi_window_sink_anyg_bf16 if any_ else built.fa2_decode_paged_multi_window_sink_bf16
        return fn(b(2, 3, Hq, 64) if q is None else q, pb() if kp is None else kp, pb(), *ints[:2], W, sinks, b(2, 3, Hq, 64) if q is None else torch.zeros_like(q))

    def pre8(W=5, sinks=None, q=None, kp=None, ks=sc):
        return built.fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8(b(40, Hq, 64) if q is None else q, p8() if kp is None else kp, p8(), *ints, ks,
                                                                        sc, W, sinks, b(40, Hq, 64) if q is None else torch.zeros_like(q))

    def dec8(W=5, sinks=None, q=None, kp=None, ks=sc):
        return built.fa2_decode_paged_multi_window_sink_anyg_bf16_fp8(b(2, 3, Hq, 64) if q is None else q, p8() if kp is None else kp, p8(), *ints[:2],
                                                                      ks, sc, W, sinks, b(2, 3, Hq, 64) if q is None else torch.zeros_like(q))

    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)  # everything here is on the CPU: the other checks are what is looked at
    for call, shape, pool in ((pre, (40, Hq, 64), torch.float16), (dec, (2, 3, Hq, 64), torch.float16), (pre8, (40, Hq, 64), BF),
                              (dec8, (2, 3, Hq, 64), BF)):
        with pytest.raises(RuntimeError, match=r"^values must be torch::k(BFloat16|Float8_e4m3fn)$"):
            call(kp=torch.zeros(9, 2, 16, 64, dtype=pool))
        with pytest.raises(RuntimeError, match=r"^values must be torch::kBFloat16$"):
            call(q=torch.zeros(*shape, dtype=torch.float16))
        for kw in ({"sinks": torch.zeros(9)}, {"sinks": torch.zeros(1, Hq)}):
            with pytest.raises(RuntimeError, match=r"^Tensor size mismatch!$"):
                call(**kw)
        with pytest.raises(RuntimeError, match=r"^values must be torch::kFloat32$"):
            call(sinks=torch.zeros(Hq, dtype=BF))
        for W in (0, -3):
            with pytest.raises(RuntimeError, match=r"window %d not supported \(>= 1\)" % W):
                call(W=W)
        with pytest.raises(RuntimeError, match=r"anyg_bf16(_fp8)?: 15 query heads are no multiple of 2 KV heads"):
            call(q=b(*shape[:-2], 15, 64))
        with pytest.raises(RuntimeError, match=r"anyg_bf16(_fp8)?: group size 17 \(= Hq 34 / Hkv 2\) not supported \(1 … 16\)"):
            call(q=b(*shape[:-2], 34, 64))
    for call in (pre8, dec8):
        with pytest.raises(RuntimeError, match=r"^Tensor size mismatch!$"):
            call(ks=torch.ones(3))
    # the siblings keep their words for the group size they refuse
    for call in (pre, dec):
        with pytest.raises(RuntimeError, match=r"sink_bf16: group size 7 \(= Hq 14 / Hkv 2\) not supported \(1, 2, 4 or 8\)"):
            call(sinks=torch.zeros(Hq), any_=False)
    # the decode's rows: T x G <= 64
    for fn, more in ((built.fa2_decode_paged_multi_window_sink_anyg_bf16, ()), (built.fa2_decode_paged_multi_window_sink_anyg_bf16_fp8, (sc, sc))):
        with pytest.raises(RuntimeError, match=r"T 5 x group size 13 = 65 query rows per KV head not supported \(at most 64\)"):
            fn(b(2, 5, 26, 64), p8() if more else pb(), p8() if more else pb(), *ints[:2], *more, 5, None, b(2, 5, 26, 64))
        with pytest.raises(RuntimeError, match=r"T 9 not supported \(1 … 8\)"):
            fn(b(2, 9, Hq, 64), p8() if more else pb(), p8() if more else pb(), *ints[:2], *more, 5, None, b(2, 9, Hq, 64))
    for plan in (built.fa2_decode_paged_multi_window_sink_anyg_bf16_plan, built.fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan):
        with pytest.raises(RuntimeError, match=r"window 0 not supported"):
            plan(2, 3, 14, 2, 4, 16, 64, 0)
        with pytest.raises(RuntimeError, match=r"T 5 x group size 16 = 80 query rows"):
            plan(2, 5, 32, 2, 4, 16, 64, 5)
        with pytest.raises(RuntimeError, match=r"group size 17 "):
            plan(2, 1, 34, 2, 4, 16, 64, 5)
        with pytest.raises(RuntimeError, match=r"15 query heads are no multiple of 2 KV heads"):
            plan(2, 1, 15, 2, 4, 16, 64, 5)
    # window = None reaches the C entries as 2^31 - 1, sinks = None as a null pointer: the C entries are replaced by a recorder
    seen = []
    monkeypatch.setattr(host, "_stream", lambda: None)
    monkeypatch.setattr(host, "_lse_fns", {n: (lambda n: lambda *a: seen.append((n, a)) or 0)(n) for n in (PRE, DEC, PRE8, DEC8)})
    sinks = torch.zeros(Hq)
    pre(None, None), dec(None, sinks), pre8(77, sinks), dec8(None, None)
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = seen
    assert (n0, n1, n2, n3) == (PRE, DEC, PRE8, DEC8)
    assert a0[-2] == INT_MAX and a1[-2] == INT_MAX and a2[-2] == 77 and a3[-2] == INT_MAX
    assert a0[6] is None and a1[5] == sinks.data_ptr() and a2[6:9] == (sc.data_ptr(), sc.data_ptr(), sinks.data_ptr()) and a3[7] is None
    assert len(a0) == 19 and len(a1) == 20 and len(a2) == 21 and len(a3) == 22
    assert a0[9:13] == (2, 40, Hq, 2) and a1[10:14] == (2, 3, Hq, 2)  # B, total_q | T, Hq, Hkv


# ---------------------------------------------------------------------------------------------------- the GPU cases see the wrong maps

def _bound_and_defects(what, q, pool, lens, cu, W, sinks, ref_o, emul, defects):
    """The model with the right map is the reference (to fp64 rounding); each defect is > 4 x the case's o_bound away."""
    bound = br.o_bound(emul, ref_o)
    right = ac.mapped(q, *pool, lens, cu, W, sinks)
    fin = torch.isfinite(ref_o)
    assert float((right[fin] - ref_o[fin]).abs().max()) <= 1e-9, what
    out = {}
    for d in defects:
        r = ac.away(ref_o, bound, ac.mapped(q, *pool, lens, cu, W, sinks, defect=d))
        assert r > 4, (what, d, r)
        out[d] = r
    return out


def test_the_gpu_cases_would_notice_the_three_wrong_row_maps():
    """tests/test_gpu_paged_anyg_attention.py's cases, on the CPU in fp64: t = r >> ceil(log2 G) on every case with G no power of two and T > 1
    (T = 1: that map IS the right one), the sink of head h 8 + g on every case with sinks, Hkv > 1 and G != 8, the slots from cu_q[b] Gpow2 / 128
    + b on the packed ragged case at G = 3, where the last sequence's slot 6 falls off the grid of 6 (at G = 7 the wrong slots 0, 3, 4, 5, 8 happen
    to fit the grid of 9 and every tile still finds its sequence: that case cannot see this defect, and is not asked to)."""
    worst = {}

    def note(got):
        for d, r in got.items():
            worst[d] = min(worst.get(d, float("inf")), r)
    D = 64  # the maps do not depend on D
    for G, page, W in itertools.product(ac.GROUPS, ac.P1_PAGES, ac.P1_WINDOWS):
        q, cu, lens, pool = ac.prefill_case(D, G, page)
        sinks = ac.sinks_for(ac.P1_HKV * G, 33)
        ro, _, emul = sr.prefill(q, *pool, lens, cu, W, sinks)
        note(_bound_and_defects(("prefill", G, page, W), q, pool, lens, cu, W, sinks, ro, emul, ("sink8",) if G == 16 else ("shift", "sink8")))
    for G in ac.P2_G:
        qs, lens, pool = ac.ragged_case(D, G)
        q, cu = sr.pack(qs)
        sinks = ac.sinks_for(ac.P2_HKV * G, ac.P2_W)
        ro, _, emul = sr.prefill(q, *pool, lens, cu, ac.P2_W, sinks)
        note(_bound_and_defects(("ragged", G), q, pool, lens, cu, ac.P2_W, sinks, ro, emul, ("shift", "sink8", "slot") if G == 3 else ("shift", "sink8")))
    for (T, G), W in itertools.product(ac.D3_TG, ac.D3_WINDOWS):
        q, lens, pool = ac.decode_one_case(T, G, D)
        B, Hq = q.shape[0], q.shape[2]
        sinks = ac.sinks_for(Hq, 33)
        ro, _, emul = sr.decode(q, *pool, lens, W, sinks)
        cu = [T * b for b in range(B + 1)]
        flat = lambda t: t.reshape(B * T, Hq, D)  # noqa: E731
        defects = (("shift",) if T > 1 and G != 16 else ()) + ("sink8",)
        note(_bound_and_defects(("decode", T, G, W), flat(q), pool, lens, cu, W, sinks, flat(ro), flat(emul), defects))
    assert set(worst) == {"shift", "sink8", "slot"}
    print("smallest wrong / bound: " + ", ".join("%s %.1f" % kv for kv in sorted(worst.items())))


# ---------------------------------------------------------------------------------------------------- registers and instructions

@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_prefill_kernels_keep_two_workgroups_per_cu_and_the_siblings_mfma_count(tmp_path, fp8):
    tail = "_bf16_fp8" if fp8 else "_bf16"
    got = fs._bodies("flash_attn_prefill_paged_varlen_window_sink_anyg%s.hip" % tail, tmp_path)
    sib = dict((k["lds"], (fs._loop_mfmas(b), k)) for k, b in fs._bodies("flash_attn_prefill_paged_varlen_window_sink%s.hip" % tail, tmp_path))
    assert len(got) == 2 and all("fa2_prefill_paged_varlen_window_sink_anyg%s_mfma" % tail in k["name"] for k, _ in got), [k["name"] for k, _ in got]
    for k, body in got:
        D = 128 if k["lds"] > 30000 else 64
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")}, "sibling:", {x: sib[k["lds"]][1][x] for x in ("vgpr", "sgpr", "lds")})
        assert 0 < 2 * k["lds"] <= fs.LDS_PER_CU and k["vgpr"] <= 256, k  # two workgroups per CU, two waves per SIMD
        assert fs._loop_mfmas(body) == D // 2 == sib[k["lds"]][0], k["name"]
        assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body and ("v_cvt_scalef32_pk_bf16_fp8" in body) == fp8, k["name"]
        assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", ""), k["name"]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_kernels_the_siblings_mfma_counts_and_the_two_combines(tmp_path, fp8):
    tail = "_bf16_fp8" if fp8 else "_bf16"
    got = fs._bodies("flash_attn_decode_paged_multi_window_sink_anyg%s.hip" % tail, tmp_path)
    stream = [(k, b) for k, b in got if "fa2_decode_paged_multi_window_sink_anyg%s_mfma" % tail in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_window_" in k["name"]]
    assert len(stream) == 8 and len(combine) == 4 and len(got) == 12, [k["name"] for k, _ in got]
    sib_bodies = [(k, b) for k, b in fs._bodies("flash_attn_decode_paged_multi_window_sink%s.hip" % tail, tmp_path) if "_mfma" in k["name"]]
    sib = sorted(fs._loop_mfmas(b) for _, b in sib_bodies)
    sib_regs = {re.search(r"ILi(\d+)ELi(\d)E", k["name"]).groups(): {x: k[x] for x in ("vgpr", "agpr", "sgpr")} for k, _ in sib_bodies}
    assert sorted(fs._loop_mfmas(b) for _, b in stream) == sib == sorted([8 * mt for mt in (1, 2, 3, 4)] + [16 * mt for mt in (1, 2, 3, 4)])
    for k, body in stream:
        m = re.search(r"ILi(\d+)ELi(\d)E", k["name"])
        D, MT = int(m.group(1)), int(m.group(2))
        # the allocation is the compiler's and may differ from the sibling's by a few registers (DESIGN 4.4.13 has both): printed, not pinned
        print(k["name"], {x: k[x] for x in ("vgpr", "agpr", "sgpr")}, "sibling:", sib_regs[m.groups()])
        assert fs._loop_mfmas(body) == (8 if D == 64 else 16) * MT, k["name"]
        assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body and ("v_cvt_scalef32_pk_bf16_fp8" in body) == fp8, k["name"]
        assert k["vgpr"] <= 512, k
    for k, body in combine:
        assert "v_cvt_pk_bf16_f32" in body and "global_store_short" in body and "v_mfma" not in body, k["name"]
