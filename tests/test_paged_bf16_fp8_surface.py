"""CPU: the bf16 paged entries over FP8 (e4m3) pools (include/cln_amd_ext.h: cln_kv_append_paged_varlen_bf16_fp8,
cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8, cln_fa2_decode_paged_multi_window_sink_bf16_fp8 with their plan / describe entries;
csrc/*_bf16_fp8.{cuh,hip}) -- the sensitivity of the GPU cases to a dropped or a neighbour's scale and to a dropped or double-counted sink,
header, exports, the plan against the window sibling's, every status code before any device access against the bf16 siblings' and then those of
the scales and of an optional `sinks`, the describe texts, the Python errors, and the kernels' resources and instructions. No GPU needed: hipcc
cross-compiles."""
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
import fp8_kv_reference as f8  # noqa: E402
import paged_bf16_fp8_reference as fr  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import paged_window_reference as wr  # noqa: E402

APPEND, APPEND_D = "cln_kv_append_paged_varlen_bf16_fp8", "cln_kv_append_paged_varlen_bf16_fp8_describe"
PREFILL, PREFILL_D = "cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8", "cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8_describe"
MULTI, MULTI_P, MULTI_D = ("cln_fa2_decode_paged_multi_window_sink_bf16_fp8", "cln_fa2_decode_paged_multi_window_sink_bf16_fp8_plan",
                           "cln_fa2_decode_paged_multi_window_sink_bf16_fp8_describe")
NAMES = (APPEND, APPEND_D, PREFILL, PREFILL_D, MULTI, MULTI_P, MULTI_D)
SIBLING = {n: n.replace("_bf16_fp8", "_bf16") for n in NAMES}  # section 17's append, section 19's attention entries
WINDOW_P = "cln_fa2_decode_paged_multi_window_bf16_plan"
LDS_PER_CU = 160 * 1024
INT_MAX = sr.INT_MAX
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------- the inputs are sensitive

def _away(ref, bound, o):
    fin = torch.isfinite(ref)
    return float((o[fin] - ref[fin]).abs().max()) / bound


def _sensitive(what, fn, q, pool, ks, vs, sinks, *mid):
    """The reference with each wrong pair of scales, and with the sink counted zero times or twice, is > 4 x the case's o_bound from the right one."""
    args = lambda a, b: (q, *pool) + mid[:-1] + (a, b, mid[-1], sinks)  # noqa: E731
    ro, _, emul = fn(*args(ks, vs))
    bound = br.o_bound(emul, ro)
    worst = float("inf")
    for name, k2, v2 in fr.wrong_scales(ks, vs):
        r = _away(ro, bound, fn(*args(k2, v2))[0])
        assert r > 4, (what, name, r)
        worst = min(worst, r)
    for count in (0, 2):
        r = _away(ro, bound, fn(*args(ks, vs), count=count)[0])
        assert r > 4, (what, "sink x %d" % count, r)
        worst = min(worst, r)
    return worst


def test_the_gpu_cases_would_notice_a_wrong_scale_or_a_wrong_sink_count():
    """Every parity case of tests/test_gpu_paged_bf16_fp8_attention.py that runs with the mixed sink set (all of them do): prefill, decode with
    one split, decode with several."""
    worst = float("inf")
    for D, (Hq, Hkv), page, W in itertools.product((64, 128), sr.PREFILL_HEADS, sr.PREFILL_PAGES, fr.PREFILL_WINDOWS):
        qs, lens, pool, ks, vs = fr.prefill_case(D, Hq, Hkv, page)
        q, cu = sr.pack(qs)
        sinks = sr.prefill_sinks(Hq, INT_MAX if W is None else W)
        worst = min(worst, _sensitive(("prefill", D, Hq, Hkv, page, W), fr.prefill, q, pool, ks, vs, sinks, lens, cu, W))
    for T, G, D in itertools.product(sr.DECODE_T, sr.DECODE_G, (64, 128)):
        q, lens, pool, ks, vs = fr.decode_one_case(T, G, D)
        worst = min(worst, _sensitive(("decode one", T, G, D), fr.decode, q, pool, ks, vs, sr.sinks_mixed(sr.ONE_HKV * G, sr.ONE_W), lens, sr.ONE_W))
    for G, D, n, W in itertools.product(fr.SPLIT_G, (64, 128), fr.SPLIT_LENS, sr.SPLIT_WINDOWS):
        q, lens, pool, ks, vs = fr.decode_split_case(G, D, n)
        worst = min(worst, _sensitive(("decode split", G, D, n, W), fr.decode, q, pool, ks, vs, sr.decode_split_sinks(G, n, W), lens, W))
    print("smallest wrong / bound: %.1f" % worst)


def test_scales_quantiser_and_the_reference_without_sinks():
    for Hkv in (1, 2, 8):
        for pow2 in (False, True):
            ks, vs = fr.scales(Hkv, pow2)
            for s in (ks, vs):
                r = s[1:] / s[:-1]
                assert bool(((r >= 2) | (r <= 0.5)).all()) and bool((s > 0).all())
    D, Hq, Hkv, page = 64, 8, 2, 16
    qs, lens, bpool = sr.prefill_case(D, Hq, Hkv, page)
    qs2, lens2, pool, ks, vs = fr.prefill_case(D, Hq, Hkv, page)
    nan = torch.isnan(bpool[0].float())
    assert bool((f8.bits(pool[0])[nan] == fr.NAN_BYTE).all()) and not bool((f8.bits(pool[0])[~nan] & 0x7F == 0x7F).any()) and bool(nan.any())
    back = fr.dq(pool[0], ks)
    assert float((back[~nan] - bpool[0].double()[~nan]).abs().max()) <= 2.0 ** -4 * float(bpool[0][~nan].abs().max())  # a half ulp of e4m3
    ks2, vs2 = fr.scales(Hkv, pow2=True)
    p2 = fr.quantize_pools(bpool, ks2, vs2)
    d = fr.dq(p2[0], ks2)
    assert torch.equal(torch.nan_to_num(d.to(BF).double()), torch.nan_to_num(d))  # power-of-two scales: the dequantised pool is a bf16 tensor
    q, cu = sr.pack(qs)
    got = fr.prefill(q, *pool, lens, cu, ks, vs, 65, None)  # sinks = None: the window reference on the dequantised pools
    want = wr.prefill(q, fr.dq(pool[0], ks), fr.dq(pool[1], vs), pool[2], lens, cu, 65)
    for a, b in zip(got, want):
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def test_append_reference_quantises_byte_for_byte():
    """mode 0: the written rows are fp8_kv_reference.quantize of the input; every other byte is what it was."""
    Hkv, D, page = 2, 64, 16
    g = torch.Generator().manual_seed(1)
    ks, vs = fr.scales(Hkv)
    k_new, v_new = (torch.randn(6, Hkv, D, generator=g).to(BF) for _ in range(2))
    bt = torch.tensor([[2, 0], [1, 3]], dtype=torch.int32)
    empty = torch.full((5, Hkv, page, D), fr.NAN_BYTE, dtype=torch.uint8).view(f8.F8)
    kb, vb, live, rows, dead = fr.ref_append(k_new, v_new, empty, empty, bt, [18, 3], [0, 2, 6], ks, vs, None, None, 0)
    assert dead == [2] and len(rows) == 5 and int(live.sum()) == 5  # sequence 1: 4 tokens, len 3: the first is not live
    assert torch.equal(kb[0, :, 0], f8.bits(f8.quantize(k_new[0], ks.reshape(-1, 1)))) and torch.equal(vb[0, :, 1], f8.bits(f8.quantize(v_new[1], vs.reshape(-1, 1))))
    assert int((kb != fr.NAN_BYTE).sum()) <= 5 * Hkv * D and bool((kb[4] == fr.NAN_BYTE).all())


# ---------------------------------------------------------------------------------------------------- header, exports, plan

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_seven_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a0)(const void*, const void*, void*, void*, const int*, const int*, const int*, const float*, const float*, const void*,"
                   " void*, const float*, int, int, int, int, int, int, int, int, int, int, void*) = %s;\n"
                   "int (*t0)(int, int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int (*a1)(const void*, const void*, const void*, const int*, const int*, const int*, const float*, const float*, const float*,"
                   " void*, float*, int, int, int, int, int, int, int, int, int, void*) = %s;\n"
                   "int (*t1)(int, int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int (*a3)(const void*, const void*, const void*, const int*, const int*, const float*, const float*, const float*, void*, float*,"
                   " void*, long long, int, int, int, int, int, int, int, int, int, void*) = %s;\n"
                   "int (*p3)(int, int, int, int, int, int, int, int, int*, int*, long long*) = %s;\n"
                   "int (*t3)(int, int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int main(void) { return a0 && t0 && a1 && t1 && a3 && p3 && t3 ? 0 : 1; }\n" % NAMES)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _fn(name, argtypes):
    fn = getattr(_lib(), name)
    fn.argtypes, fn.restype = argtypes, ctypes.c_int
    return fn


def _plan(name, *dims):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_void_p] * 3)
    s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    rc = fn(*dims, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
    return rc, (s.value, c.value, w.value)


def _describe(name, *dims):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(*dims, buf, 4096)
    return rc, buf.value.decode()


def test_library_header_and_package_hold_the_entries(built):
    lib, hdr = _lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ("kv_append_paged_varlen_bf16_fp8", "fa2_prefill_paged_varlen_window_sink_bf16_fp8", "fa2_decode_paged_multi_window_sink_bf16_fp8",
              "fa2_decode_paged_multi_window_sink_bf16_fp8_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    for n in ("describe_kv_append_paged_varlen_bf16_fp8", "describe_prefill_paged_varlen_window_sink_bf16_fp8",
              "describe_decode_paged_multi_window_sink_bf16_fp8"):
        assert hasattr(built.manifest, n), n
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:  # none of the new names is a manifest name
        assert n not in names and n.replace("cln_", "") not in names


def test_plan_is_the_window_plan_status_included(built):
    n = split = 0
    for B, T, (Hq, Hkv), (mp, page), D, W in itertools.product((1, 5, 64), (1, 3, 8), ((1, 1), (8, 1), (64, 8)),
                                                               ((19, 16), (256, 16), (1024, 16), (64, 256)), (64, 128),
                                                               (1, 33, 128, 1000, 4096, 1 << 20, INT_MAX)):
        got = _plan(MULTI_P, B, T, Hq, Hkv, mp, page, D, W)
        assert got[0] == 0 and got == _plan(WINDOW_P, B, T, Hq, Hkv, mp, page, D, W), (B, T, Hq, Hkv, mp, page, D, W)
        assert got[1] == wr.plan(B, T, Hq, Hkv, mp, page, D, W) == built.fa2_decode_paged_multi_window_sink_bf16_fp8_plan(B, T, Hq, Hkv, mp, page, D, W)
        n += 1
        split += got[1][0] > 1
    assert n > 1000 and split > 100
    for B, T, Hq, Hkv, mp, page, D in ((1, 1, 8, 1, 1024, 16, 64), (5, 8, 64, 8, 256, 16, 128)):  # window = None: no window
        assert (built.fa2_decode_paged_multi_window_sink_bf16_fp8_plan(B, T, Hq, Hkv, mp, page, D, None)
                == built.fa2_decode_paged_multi_window_bf16_plan(B, T, Hq, Hkv, mp, page, D, INT_MAX))
    for dims in ((0, 2, 8, 8, 4, 16, 64), (1, 9, 8, 8, 4, 16, 64), (1, 2, 8, 3, 4, 16, 64), (1, 2, 8, 8, 4, 16, 96), (1, 2, 8, 8, 4, 48, 64)):
        for W in (5, 0):
            assert _plan(MULTI_P, *dims, W) == _plan(WINDOW_P, *dims, W)
            for name in (PREFILL_D, MULTI_D):
                a, b = _describe(name, *dims, W)[0], _describe(SIBLING[name], *dims, W)[0]
                assert min(a, 0) == min(b, 0), (name, dims, W, a, b)


# ---------------------------------------------------------------------------------------------------- status codes
# Never dereferenced: every call below fails its checks first.

SINKS, KS, VS = 0x10000 * 20, 0x10000 * 21, 0x10000 * 22
INT9 = [ctypes.c_int] * 9


def _statuses(f, g, n_in, n_out, tail, dims, bad_d):
    """f: the new entry (inputs, k_scale, v_scale, sinks, outputs), g: the section 19 sibling (inputs, sinks, outputs). The sibling's status for
    the same arguments; then the scales where a bad last input is; then sinks: NULL legal, misaligned or an output -1."""
    p = [0x10000 * (i + 1) for i in range(n_in + n_out)]

    def new(ptrs, d, sinks=SINKS, ks=KS, vs=VS, W=5):
        return f(*ptrs[:n_in], ks, vs, sinks, *ptrs[n_in:], *tail, *d, W, None)

    def both(ptrs, d, want, W=5):
        a, b = new(ptrs, d, W=W), g(*ptrs[:n_in], SINKS, *ptrs[n_in:], *tail, *d, W, None)
        assert a == b == want, (ptrs, d, W, a, b)
        assert new(ptrs, d, None, W=W) == want  # ... and without sinks
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
    a = list(p)
    a[n_in - 1] = None  # what a bad last input gives: a bad scale gives the same, before the shape
    for d in (dims, bad_d):
        want = g(*a[:n_in], SINKS, *a[n_in:], *tail, *d, 5, None)
        assert want == -1
        for kw in ({"ks": None}, {"vs": None}, {"ks": KS + 2}, {"vs": VS + 1}, {"ks": p[n_in]}, {"vs": p[n_in]}):
            assert new(p, d, **kw) == -1, (kw, d)
            assert new(p, d, None, **kw) == -1, (kw, d)
        for bad in (SINKS + 1, SINKS + 2) + tuple(p[n_in:]):  # sinks: misaligned, or an output
            assert new(p, d, bad) == -1, (bad, d)
    assert new(p, bad_d, SINKS + 4, KS + 4, VS + 4) == -2  # 4-byte alignment is enough: the shape is looked at
    assert new(p, bad_d, None) == -2


def test_prefill_statuses_are_the_sink_siblings_then_those_of_the_scales_and_of_optional_sinks(built):
    f = _fn(PREFILL, [ctypes.c_void_p] * 11 + INT9 + [ctypes.c_void_p])
    g = _fn(SIBLING[PREFILL], [ctypes.c_void_p] * 9 + INT9 + [ctypes.c_void_p])
    dims = (3, 170, 8, 2, 40, 6, 16, 128)  # B, total_q, Hq, Hkv, P, max_pages, page, D
    _statuses(f, g, 6, 2, (), dims, dims[:7] + (96,))
    for d in ((3, 170, 8, 3, 40, 6, 16, 128), ):
        assert f(*[0x10000 * (i + 1) for i in range(6)], KS, VS, None, 0x70000, 0x80000, *d, 5, None) == -1  # Hq % Hkv
    for d in ((3, 170, 6, 2, 40, 6, 16, 128), (3, 170, 8, 2, 40, 6, 48, 128), (3, 170, 8, 2, 40, 1 << 23, 256, 128), (1, 1 << 28, 8, 1, 40, 6, 16, 128)):
        assert f(*[0x10000 * (i + 1) for i in range(6)], KS, VS, SINKS, 0x70000, 0x80000, *d, 5, None) == -2


def test_multi_statuses_are_the_sink_siblings_then_those_of_the_scales_and_of_optional_sinks(built):
    f = _fn(MULTI, [ctypes.c_void_p] * 11 + [ctypes.c_longlong] + INT9 + [ctypes.c_void_p])
    g = _fn(SIBLING[MULTI], [ctypes.c_void_p] * 9 + [ctypes.c_longlong] + INT9 + [ctypes.c_void_p])
    dims = (3, 4, 8, 2, 40, 6, 16, 128)  # B, T, Hq, Hkv, P, max_pages, page, D: one split, no workspace needed
    _statuses(f, g, 5, 3, (1 << 30,), dims, dims[:7] + (96,))
    p = [0x10000 * (i + 1) for i in range(8)]
    for d in ((3, 9, 8, 2, 40, 6, 16, 128), (3, 4, 6, 2, 40, 6, 16, 128), (3, 4, 8, 2, 40, 6, 48, 128), (3, 4, 8, 2, 40, 1 << 23, 256, 128)):
        assert f(*p[:5], KS, VS, None, *p[5:], 1 << 30, *d, 5, None) == -2
    split = (1, 2, 4, 1, 40, 256, 16, 128)  # max_pages page = 4096 and W = 1000: 3 splits, the workspace is required, and large enough
    rc, (S, C, need) = _plan(MULTI_P, *split[:4], *split[5:], 1000)
    assert rc == 0 and (S, C) == (3, 384) and need == 1 * 2 * 4 * 3 * 130 * 4
    for sinks in (SINKS, None):
        assert f(*p[:5], KS, VS, sinks, *p[5:7], None, 0, *split, 1000, None) == -1
        assert f(*p[:5], KS, VS, sinks, *p[5:], need - 1, *split, 1000, None) == -1


def test_append_statuses_are_those_of_the_bf16_append_then_those_of_the_scales(built):
    """k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q | k_scale, v_scale | q, q_out, rope_table; B, total_q, Hq, Hkv, P, max_pages,
    page, D, max_pos, rope_mode."""
    INT10 = [ctypes.c_int] * 10
    f = _fn(APPEND, [ctypes.c_void_p] * 12 + INT10 + [ctypes.c_void_p])
    g = _fn(SIBLING[APPEND], [ctypes.c_void_p] * 10 + INT10 + [ctypes.c_void_p])
    p = [0x10000 * (i + 1) for i in range(10)]
    dims = (3, 170, 8, 2, 40, 6, 16, 128, 96, 1)

    def both(ptrs, d, want):
        a, b = f(*ptrs[:7], KS, VS, *ptrs[7:], *d, None), g(*ptrs, *d, None)
        assert a == b == want, (ptrs, d, a, b)
    both(p, dims[:7] + (96, 96, 1), -2)
    both(p, dims[:9] + (3,), -2)
    for i in range(10):
        a = list(p)
        a[i] = None
        both(a, dims, -1)
        a[i] = p[i] + 2
        both(a, dims, -1)
    a = list(p)
    a[8] = p[7]  # q_out may be q ...
    both(a, dims[:7] + (96, 96, 1), -2)
    for out in (2, 3, 8):  # ... and no other output is an input or another output
        for src in range(10):
            if src != out and (out, src) != (8, 7):
                a = list(p)
                a[out] = p[src]
                both(a, dims, -1)
    for i in range(9):
        d = list(dims)
        d[i] = 0
        both(p, d, -1)
    both(p, dims[:9] + (0,), -1)  # rope none takes no q, q_out or rope_table
    for d in (dims, dims[:7] + (96, 96, 1)):  # the scales: null, misaligned, an output -- -1 where a bad cu_q is, before the shape
        a = list(p)
        a[6] = None
        assert g(*a, *d, None) == -1
        for ks, vs in ((None, VS), (KS, None), (KS + 2, VS), (KS, VS + 1), (p[2], VS), (KS, p[3]), (KS, p[8])):
            assert f(*p[:7], ks, vs, *p[7:], *d, None) == -1, (ks, vs, d)
    assert f(*p[:7], KS + 4, VS + 4, *p[7:], *dims[:7], 96, 96, 1, None) == -2


# ---------------------------------------------------------------------------------------------------- describe, Python errors

def test_describe_texts_match_the_python_mirrors(built):
    m = built.manifest
    splits = set()
    for D, G, page, W in itertools.product((64, 128), pr.GROUPS, (16, 64, 256), (1, 128, 1024, INT_MAX)):
        for (B, tq, Hkv, mp) in ((1, 1, 1, 1), (5, 204, 1, 32), (65, 2112, 8, 300)):
            Hq = Hkv * G
            rc, text = _describe(PREFILL_D, B, tq, Hq, Hkv, mp, page, D, W)
            assert rc == len(text) > 0, (rc, text)
            assert text == m.describe_prefill_paged_varlen_window_sink_bf16_fp8(B, tq, Hq, Hkv, mp, page, D, W)
            assert text == fr.describe_prefill_text(B, tq, Hq, Hkv, mp, page, D, W)
            assert text.startswith("fa2_prefill_paged_varlen_window_sink_bf16_fp8_mfma<D=%d,G=%d> B=%d" % (D, G, B))
            assert "v_cvt_scalef32_pk_bf16_fp8, exact" in text and "times k_scale" in text and "times v_scale" in text and "_f16" not in text
            assert "(fp32, natural log, unscaled; none when sinks is NULL)" in text
        for (B, T, Hkv, mp) in ((1, 1, 1, 256), (7, 3, 2, 19), (64, 8, 8, 300), (1, 8, 1, 4096)):
            Hq = Hkv * G
            rc, text = _describe(MULTI_D, B, T, Hq, Hkv, mp, page, D, W)
            assert rc == len(text) > 0, (rc, text)
            assert text == m.describe_decode_paged_multi_window_sink_bf16_fp8(B, T, Hq, Hkv, mp, page, D, W)
            assert text == fr.describe_multi_text(B, T, Hq, Hkv, mp, page, D, W)
            S = wr.plan(B, T, Hq, Hkv, mp, page, D, W)[0]
            splits.add(S > 1)
            assert text.startswith("fa2_decode_paged_multi_window_sink_bf16_fp8_mfma<D=%d,MT=%d> T=%d G=%d W=%d " % (D, -(-T * G // 16), T, G, W))
            assert "v_cvt_scalef32_pk_bf16_fp8, exact" in text and "times k_scale" in text and "the partial times v_scale" in text
            assert ("fa2_decode_combine_window_sink_bf16_rows<D=%d>" % D in text) == (S > 1) and "none when sinks is NULL" in text
        for mode, (B, tq, Hkv) in itertools.product((0, 1, 2), ((1, 1, 1), (5, 204, 2), (65, 2112, 8))):
            Hq = Hkv * G
            rc, text = _describe(APPEND_D, B, tq, Hq, Hkv, 32, page, D, mode)
            assert rc == len(text) > 0, (rc, text)
            assert text == m.describe_kv_append_paged_varlen_bf16_fp8(B, tq, Hq, Hkv, 32, page, D, ("none", "half", "interleaved")[mode])
            assert text == fr.describe_append_text(B, tq, Hq, Hkv, 32, page, D, mode)
    assert splits == {False, True}
    with pytest.raises(ValueError):
        m.describe_prefill_paged_varlen_window_sink_bf16_fp8(3, 8, 8, 2, 40, 16, 128, 0)
    with pytest.raises(ValueError):
        m.describe_decode_paged_multi_window_sink_bf16_fp8(1, 9, 8, 8, 4, 16, 64, 5)
    with pytest.raises(ValueError):
        m.describe_kv_append_paged_varlen_bf16_fp8(1, 9, 8, 8, 4, 16, 64, "spiral")


def test_python_entries_refuse_bad_tensors_before_any_device_call_and_forward_none(built, monkeypatch):
    from cuda_learn_notes_amd import host
    i32 = torch.int32
    ints = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32))
    b = lambda *s: torch.zeros(*s, dtype=BF)  # noqa: E731
    p8 = lambda: torch.zeros(9, 2, 16, 64, dtype=torch.uint8).view(f8.F8)  # noqa: E731
    sc = torch.ones(2)

    def pre(W=5, sinks=None, q=None, kp=None, ks=sc, vs=sc):
        return built.fa2_prefill_paged_varlen_window_sink_bf16_fp8(b(40, 8, 64) if q is None else q, p8() if kp is None else kp, p8(), *ints, ks, vs, W,
                                                                   sinks, b(40, 8, 64))

    def dec(W=5, sinks=None, q=None, kp=None, ks=sc, vs=sc):
        return built.fa2_decode_paged_multi_window_sink_bf16_fp8(b(2, 3, 8, 64) if q is None else q, p8() if kp is None else kp, p8(), *ints[:2], ks, vs,
                                                                 W, sinks, b(2, 3, 8, 64))

    def app(kn=None, kp=None, ks=sc, vs=sc):
        return built.kv_append_paged_varlen_bf16_fp8(b(40, 2, 64) if kn is None else kn, b(40, 2, 64), p8() if kp is None else kp, p8(), *ints, ks, vs)

    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)  # everything here is on the CPU: the other checks are what is looked at
    for call, shape in ((pre, (40, 8, 64)), (dec, (2, 3, 8, 64))):
        with pytest.raises(RuntimeError, match=r"^values must be torch::kFloat8_e4m3fn$"):
            call(kp=b(9, 2, 16, 64))
        with pytest.raises(RuntimeError, match=r"^values must be torch::kBFloat16$"):
            call(q=torch.zeros(*shape, dtype=torch.float16))
        for kw in ({"ks": torch.ones(2, dtype=torch.float64)}, {"vs": torch.ones(2, dtype=BF)}):
            with pytest.raises(RuntimeError, match=r"^values must be torch::kFloat32$"):
                call(**kw)
        for kw in ({"ks": torch.ones(3)}, {"vs": torch.ones(1, 2)}, {"sinks": torch.zeros(9)}, {"sinks": torch.zeros(1, 8)}):
            with pytest.raises(RuntimeError, match=r"^Tensor size mismatch!$"):
                call(**kw)
        with pytest.raises(RuntimeError, match=r"^values must be torch::kFloat32$"):
            call(sinks=torch.zeros(8, dtype=BF))
        for W in (0, -3):
            with pytest.raises(RuntimeError, match=r"window %d not supported \(>= 1\)" % W):
                call(W=W)
    with pytest.raises(RuntimeError, match=r"^values must be torch::kFloat8_e4m3fn$"):
        app(kp=b(9, 2, 16, 64))
    with pytest.raises(RuntimeError, match=r"^values must be torch::kBFloat16$"):
        app(kn=torch.zeros(40, 2, 64, dtype=torch.float16))
    with pytest.raises(RuntimeError, match=r"^Tensor size mismatch!$"):
        app(ks=torch.ones(3))
    with pytest.raises(RuntimeError, match=r"fa2_decode_paged_multi_window_sink_bf16_fp8: window 0 not supported"):
        built.fa2_decode_paged_multi_window_sink_bf16_fp8_plan(2, 3, 8, 2, 4, 16, 64, 0)
    # window = None reaches the C entries as 2^31 - 1, sinks = None as a null pointer behind the scales: the C entries are replaced by a recorder
    seen = []
    monkeypatch.setattr(host, "_stream", lambda: None)
    monkeypatch.setattr(host, "_lse_fns", {"cln_" + n: (lambda n: lambda *a: seen.append((n, a)) or 0)(n) for n in (
        "fa2_prefill_paged_varlen_window_sink_bf16_fp8", "fa2_decode_paged_multi_window_sink_bf16_fp8", "kv_append_paged_varlen_bf16_fp8")})
    sinks = torch.zeros(8)
    pre(None, None), dec(None, sinks), pre(77, sinks), app()
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = seen
    assert a0[-2] == INT_MAX and a1[-2] == INT_MAX and a2[-2] == 77
    assert a0[6:9] == (sc.data_ptr(), sc.data_ptr(), None) and a2[8] == sinks.data_ptr() and a1[5:8] == (sc.data_ptr(), sc.data_ptr(), sinks.data_ptr())
    assert len(a0) == 21 and len(a1) == 22 and len(a3) == 23 and a3[7:9] == (sc.data_ptr(), sc.data_ptr()) and a3[9:12] == (None, None, None)


# ---------------------------------------------------------------------------------------------------- registers and instructions

def _bodies(src, tmp_path):
    import kernel_resources as kres
    kernels, s = kres.report(os.path.join(CSRC, src), keep=str(tmp_path))
    text = open(s).read()
    out = []
    for k in kernels:
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        out.append((k, body))
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert not k["name"].endswith("_kernel") and "_kernelI" not in k["name"], k["name"]
        assert "_f16" not in body and "atomic" not in body, k["name"]  # no fp16 MFMA, no conversion through fp16
    return out


def _loop_mfmas(body):
    """The MFMAs of the kernel's key loop -- the one loop that holds any: those in the basic blocks the compiler's comments place in it (the
    header `=>This Inner Loop Header`, the others `in Loop: Header=<the same block>`; a block label without either is outside every loop). The
    kernel has none outside it, asserted here."""
    loops, cur, name, label = {}, None, None, False
    for line in body.splitlines():
        m = re.match(r"\.(LBB\d+_\d+):(.*)", line)
        if m:
            name, cur, label = m.group(1), None, True  # the comments of a named block follow on lines of their own
        if label and (m or line.lstrip().startswith(";")):
            h = re.search(r"in Loop: Header=(?:LBB|BB)(\d+_\d+)", line)
            cur = name if "Loop Header" in line else "LBB" + h.group(1) if h else cur
            continue
        label = False
        if "v_mfma_f32_16x16x32_bf16" in line:
            loops[cur] = loops.get(cur, 0) + 1
    inside = {k: v for k, v in loops.items() if k is not None}
    assert None not in loops and len(inside) == 1, loops  # every MFMA is in one loop
    assert sum(inside.values()) == body.count("v_mfma_f32_16x16x32_bf16")
    return sum(inside.values())


def test_prefill_kernels_keep_two_workgroups_per_cu_and_the_siblings_mfma_count(tmp_path):
    got = _bodies("flash_attn_prefill_paged_varlen_window_sink_bf16_fp8.hip", tmp_path)
    sib = dict((k["lds"], _loop_mfmas(b)) for k, b in _bodies("flash_attn_prefill_paged_varlen_window_sink_bf16.hip", tmp_path))
    assert len(got) == 2 and all("fa2_prefill_paged_varlen_window_sink_bf16_fp8_mfma" in k["name"] for k, _ in got), [k["name"] for k, _ in got]
    for k, body in got:
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")})
        D = 128 if k["lds"] > 30000 else 64
        assert 0 < 2 * k["lds"] <= LDS_PER_CU and k["vgpr"] <= 256, k  # two workgroups per CU, two waves per SIMD
        assert _loop_mfmas(body) == D // 2 == sib[k["lds"]], k["name"]  # 32 / 64 per step, the bf16 sink sibling's
        assert "v_cvt_scalef32_pk_bf16_fp8" in body and "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]
        assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", ""), k["name"]


def test_decode_kernels_the_siblings_mfma_counts_and_the_two_combines(tmp_path):
    got = _bodies("flash_attn_decode_paged_multi_window_sink_bf16_fp8.hip", tmp_path)
    stream = [(k, b) for k, b in got if "fa2_decode_paged_multi_window_sink_bf16_fp8_mfma" in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_window_" in k["name"]]
    assert len(stream) == 8 and len(combine) == 4 and len(got) == 12, [k["name"] for k, _ in got]
    sib = [b for k, b in _bodies("flash_attn_decode_paged_multi_window_sink_bf16.hip", tmp_path) if "_mfma" in k["name"]]
    assert sorted(_loop_mfmas(b) for _, b in stream) == sorted(_loop_mfmas(b) for b in sib) == sorted([8 * mt for mt in (1, 2, 3, 4)]
                                                                                                      + [16 * mt for mt in (1, 2, 3, 4)])
    for k, body in stream:
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")})
        m = re.search(r"ILi(\d+)ELi(\d)E", k["name"])
        D, MT = int(m.group(1)), int(m.group(2))
        assert _loop_mfmas(body) == (8 if D == 64 else 16) * MT, k["name"]
        assert "v_cvt_scalef32_pk_bf16_fp8" in body and "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]
        assert k["vgpr"] <= 512, k
    for k, body in combine:
        assert "v_cvt_pk_bf16_f32" in body and "global_store_short" in body and "v_mfma" not in body, k["name"]


def test_append_kernels_quantise_without_spill_or_scratch(tmp_path):
    got = _bodies("kv_append_paged_varlen_bf16_fp8.hip", tmp_path)
    assert len(got) == 6 and all("kv_append_paged_varlen_bf16_fp8_rows" in k["name"] for k, _ in got), [k["name"] for k, _ in got]
    for k, body in got:
        assert "v_cvt_pk_fp8_f32" in body and k["lds"] == 0, k["name"]
