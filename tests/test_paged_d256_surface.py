"""CPU: the head-dim-256 entries of the bf16 paged path (include/cln_amd_ext.h: cln_kv_append_paged_varlen_d256_bf16,
cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16, cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16 with their plan /
describe entries; csrc/*_d256_bf16.{cuh,hip}) -- header, exports and package, the plan against a restatement of its rule, the
refusals and the order of the status codes against the D = 128 siblings, the Python entries, the describe texts and the kernels' resources and
MFMA counts. No GPU needed: hipcc cross-compiles."""
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
import paged_sink_reference as sr  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of a code object)

APP = "cln_kv_append_paged_varlen_d256_bf16"
PRE = "cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16"
DEC = "cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16"
NAMES = (APP, APP + "_describe", PRE, PRE + "_describe", DEC + "_plan", DEC, DEC + "_describe")
SIB = lambda n: n.replace("_d256_", "_")  # noqa: E731  the D = 64 / 128 sibling
INT_MAX = sr.INT_MAX
NAN, INF = float("nan"), float("inf")
BAD = (-1.0, NAN, INF, -INF, -1e-30)
KEY_STEP, MAX_ROWS = 64, 32  # the decode kernel's workgroup step (4 waves x one 16-key block) and its two 16-row tiles
_fn, _plan = fs._fn, fs._plan


def _describe(name, *dims, scale=0.0, cap=0.0):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_float] * 2 + [ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(*dims, scale, cap, buf, 4096)
    return rc, buf.value.decode()


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_seven_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    app = "const void*, const void*, void*, void*, const int*, const int*, const int*, const void*, void*, const float*, " + "int, " * 10 + "void*"
    app_d = "int, int, int, int, int, int, int, int, char*, int"
    pre = "const void*, const void*, const void*, const int*, const int*, const int*, const float*, void*, float*, " + "int, " * 9 + "float, float, void*"
    dec = ("const void*, const void*, const void*, const int*, const int*, const float*, void*, float*, void*, long long, " + "int, " * 9
           + "float, float, void*")
    text, plan = "int, int, int, int, int, int, int, int, float, float, char*, int", "int, int, int, int, int, int, int, int, int*, int*, long long*"
    protos = (app, app_d, pre, text, plan, dec, text)
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip(protos, NAMES)))
                   + "int main(void) { return f0 && f6 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_package_and_build_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in (APP, PRE, DEC, DEC + "_plan"):
        assert hasattr(built, n[4:]) and hasattr(host, n[4:]), n
    m = built.manifest
    assert hasattr(m, "describe_kv_append_paged_varlen_d256_bf16")
    for n in (PRE, DEC):
        assert hasattr(m, "describe_" + n[len("cln_fa2_"):]), n
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    for unit in ("kv_append_paged_varlen_d256_bf16", "flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16",
                 "flash_attn_decode_paged_multi_window_sink_softcap_anyg_d256_bf16"):
        assert '"%s.hip"' % unit in build and os.path.exists(os.path.join(fs.CSRC, unit + ".hip")), unit


# ---------------------------------------------------------------------------------------------------- plan

def plan_rule(B, T, Hq, Hkv, max_pages, page, W, D=256):
    """fa2d::split_plan on this kernel's numbers, restated: bk = B Hkv (sequence, KV head) pairs, the unit U = max(page, 64), the span
    min(Nmax, round_up(W + T - 1, U) + U) of paged::multi_window_span, split until bk S reaches 1024 workgroups but into chunks of at least 256
    keys and at most 64 splits; chunk a multiple of U; workspace rows S (D + 2) 4 bytes when S > 1."""
    Nmax, U = max_pages * page, max(page, KEY_STEP)
    span = min(Nmax, (W + T - 1 + U - 1) // U * U + U)
    bk, want = B * Hkv, 1
    if bk < 1024 and span > 256:
        want = min((1024 + bk - 1) // bk, span // 256, 64)
    chunk = ((span + want - 1) // want + U - 1) // U * U
    splits = (span + chunk - 1) // chunk
    return splits, chunk, (B * T * Hq * splits * (D + 2) * 4 if splits > 1 else 0)


def test_plan_is_the_rule_restated(built):
    n = split = 0
    for B, (T, G), Hkv, (mp, page), W in itertools.product((1, 5, 64), ((1, 1), (1, 3), (8, 4), (2, 16), (3, 5), (8, 1), (4, 8)), (1, 2, 8),
                                                           ((19, 16), (256, 16), (1024, 16), (64, 256), (100, 64)),
                                                           (1, 33, 1000, 4096, INT_MAX)):
        Hq = G * Hkv
        got = _plan(DEC + "_plan", B, T, Hq, Hkv, mp, page, 256, W)
        assert got == (0, plan_rule(B, T, Hq, Hkv, mp, page, W)), (B, T, Hq, Hkv, mp, page, W, got)
        assert got[1][1] % max(page, KEY_STEP) == 0 and got[1][0] * got[1][1] >= min(mp * page, W + T - 1)
        assert built.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(B, T, Hq, Hkv, mp, page, 256, None if W == INT_MAX else W) == got[1]
        n += 1
        split += got[1][0] > 1
    assert n > 1000 and split > 100, (n, split)


def test_plan_refusals_and_the_siblings_statuses(built):
    p = lambda *dims: _plan(DEC + "_plan", *dims)[0]  # noqa: E731
    for D in (64, 128, 96):
        assert p(1, 2, 8, 8, 4, 16, D, 5) == -2, D
    assert p(1, 3, 11, 1, 4, 16, 256, 5) == -2 and p(1, 2, 16, 1, 4, 16, 256, 5) == 0  # T G = 33, and 32
    assert p(1, 1, 17, 1, 4, 16, 256, 5) == -2 and p(1, 9, 1, 1, 4, 16, 256, 5) == -2  # G = 17, T = 9
    assert p(1, 2, 8, 8, 4, 16, 256, 0) == -1  # window = 0
    # every other status is the D = 128 sibling's for that argument
    for dims in ((0, 2, 8, 8, 4, 16), (1, 0, 8, 8, 4, 16), (1, 2, 8, 3, 4, 16), (1, 2, 8, 8, 4, 48), (1, 2, 8, 8, 1 << 23, 256), (1, 2, 0, 8, 4, 16),
                 (1, 2, 8, 8, 0, 16), (1, 2, 8, 8, 4, 16)):
        for W in (5, 0, -3):
            assert p(*dims, 256, W) == _plan(SIB(DEC) + "_plan", *dims, 128, W)[0], (dims, W)
    with pytest.raises(RuntimeError, match=r"T 5 x group size 7 = 35 query rows per KV head not supported \(at most 32\)"):
        built.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(1, 5, 7, 1, 4, 16, 256, 5)
    with pytest.raises(RuntimeError, match=r"head dim 128 not supported \(256\)"):
        built.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(1, 2, 8, 8, 4, 16, 128, 5)
    with pytest.raises(RuntimeError, match=r"group size 17 "):
        built.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(1, 1, 17, 1, 4, 16, 256, 5)
    with pytest.raises(RuntimeError, match=r"T 9 not supported"):
        built.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(1, 9, 1, 1, 4, 16, 256, 5)


# ---------------------------------------------------------------------------------------------------- statuses of the entries

def test_entries_check_the_floats_first_then_as_the_siblings(built):
    """Never dereferenced: every call here fails a check before the launch. A bad float is -1 whatever else is wrong; D = 64, 128, 96 are -2; and
    with one argument wrong at a time -- a null or misaligned pointer, an output that is an input, P, each dimension, the window, the workspace --
    the status at D = 256 is the sibling's at D = 128 for the same arguments."""
    p = [0x10000 * (i + 1) for i in range(9)]
    i9, fl = [ctypes.c_int] * 9, [ctypes.c_float] * 2
    for name, tail, lead in ((PRE, (), (3, 170)), (DEC, (1 << 40,), (3, 4))):
        sig = [ctypes.c_void_p] * 9 + [ctypes.c_longlong] * len(tail) + i9 + fl + [ctypes.c_void_p]
        f, g = _fn(name, sig), _fn(SIB(name), sig)
        good = (*lead, 8, 2, 40, 6, 16)  # B, total_q | T, Hq, Hkv, P, max_pages, page: T G = 16 rows for the decode
        for D in (64, 128, 96):
            assert f(*p, *tail, *good, D, 5, 0.0, 0.0, None) == -2, (name, D)
        for bad in BAD:
            for D in (256, 96):
                assert f(*p, *tail, *good, D, 5, bad, 0.0, None) == -1 and f(*p, *tail, *good, D, 5, 0.0, bad, None) == -1, (name, bad)
            assert f(None, *p[1:], *tail, *good, 256, 0, bad, 0.0, None) == -1
        both = lambda ps, dims, W, t=tail: (f(*ps, *t, *dims, 256, W, 0.125, 50.0, None), g(*ps, *t, *dims, 128, W, 0.125, 50.0, None))  # noqa: E731
        seen = set()
        for W in (0, -7):  # the window
            assert both(p, good, W) == (-1, -1)
        for i, v in ((0, 0), (1, 0), (2, 9), (2, 34), (3, 0), (4, 0), (5, 0), (6, 48), (6, 0), (5, 1 << 27)):  # one dimension wrong (the last: max_pages page = 2^31)
            a, b = both(p, good[:i] + (v,) + good[i + 1:], 5)
            assert a == b and a in (-1, -2), (name, i, v, a, b)
            seen.add(a)
        nullable = (5, 7, 8) if name == DEC else (6, 8)  # sinks, lse and, with one split, the workspace: NULL is taken, the call would launch
        outputs = (6, 7, 8) if name == DEC else (7, 8)
        for i in range(9):  # one pointer wrong: null, misaligned, an output that is an input
            for v in (None, p[i] + 2, p[0]):
                if (v is None and i in nullable) or (v == p[0] and i not in outputs):
                    continue
                a, b = both(p[:i] + [v] + p[i + 1:], good, 5)
                assert a == b == -1, (name, i, v, a, b)
        assert seen == {-1, -2}, seen
    # the decode's own limits, and a workspace that is too small for a plan that splits
    sig = [ctypes.c_void_p] * 9 + [ctypes.c_longlong] + i9 + fl + [ctypes.c_void_p]
    f, g = _fn(DEC, sig), _fn(SIB(DEC), sig)
    for T, Hq in ((3, 22), (9, 2), (1, 34)):  # T G = 33, T = 9, G = 17
        assert f(*p, 1 << 40, 3, T, Hq, 2, 40, 6, 16, 256, 5, 0.0, 0.0, None) == -2, (T, Hq)
    big = (3, 4, 8, 2, 40, 256, 16)
    assert _plan(DEC + "_plan", *big[:4], *big[5:], 256, INT_MAX)[1][0] > 1
    assert f(*p, 8, *big, 256, INT_MAX, 0.0, 0.0, None) == g(*p, 8, *big, 128, INT_MAX, 0.0, 0.0, None) == -1
    assert f(*p[:8], None, 1 << 40, *big, 256, INT_MAX, 0.0, 0.0, None) == -1
    # the append: D = 64, 128, 96 are -2; every other status is the bf16 sibling's at D = 128
    sig = [ctypes.c_void_p] * 10 + [ctypes.c_int] * 10 + [ctypes.c_void_p]
    f, g = _fn(APP, sig), _fn(SIB(APP), sig)
    q10 = [0x10000 * (i + 1) for i in range(10)]
    good = (3, 40, 12, 2, 40, 6, 16)  # B, total_q, Hq, Hkv, P, max_pages, page
    for D in (64, 128, 96):
        assert f(*q10, *good, D, 100, 1, None) == -2, D
    for i, v in ((0, 0), (1, 0), (2, 13), (3, 0), (4, 0), (5, 0), (6, 48)):
        dims = good[:i] + (v,) + good[i + 1:]
        a, b = f(*q10, *dims, 256, 100, 1, None), g(*q10, *dims, 128, 100, 1, None)
        assert a == b and a in (-1, -2), (dims, a, b)
    for mode, max_pos in ((1, 0), (3, 100), (-1, 100), (0, 100)):  # no table rows, no such mode, mode 0 with q / q_out / rope_table
        a, b = f(*q10, *good, 256, max_pos, mode, None), g(*q10, *good, 128, max_pos, mode, None)
        assert a == b and a in (-1, -2), (mode, max_pos, a, b)
    for i in (0, 1, 2, 3, 4, 5, 6):  # the required pointers: null, misaligned
        for v in (None, q10[i] + 2):
            ps = q10[:i] + [v] + q10[i + 1:]
            assert f(*ps, *good, 256, 100, 1, None) == g(*ps, *good, 128, 100, 1, None) == -1, (i, v)


def test_describe_texts_name_the_instantiation_the_tile_the_step_the_lds_and_the_plan(built):
    m = built.manifest
    dims = (3, 170, 12, 4, 6, 16, 256, 33)
    for bad in BAD:
        for name in (PRE, DEC):
            d = (3, 4) + dims[2:] if name == DEC else dims
            assert _describe(name + "_describe", *d, scale=bad)[0] == -1 and _describe(name + "_describe", *d, cap=bad)[0] == -1
            assert _describe(name + "_describe", *d[:6], 128, 33, scale=bad)[0] == -1
    for D in (64, 128, 96):
        assert _describe(PRE + "_describe", *dims[:6], D, 33)[0] == -2 and _describe(DEC + "_describe", 3, 4, 12, 4, 6, 16, D, 33)[0] == -2
    assert _describe(PRE + "_describe", *dims[:7], 0)[0] == -1
    for scale, cap in ((0.0, 0.0), (0.0, 50.0), (1.0 / 16, 50.0)):
        rc, text = _describe(PRE + "_describe", *dims, scale=scale, cap=cap)
        assert rc == len(text) > 0, (rc, text)
        assert text.startswith("fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_mfma<D=256,CAP=%d> softmax_scale=0.0625" % (cap != 0)), text
        assert "rows=128 keys=64" in text and "69632 bytes of static LDS" in text and "v_mfma_f32_16x16x32_bf16" in text
        assert ("capped before the window and causal mask" in text) == (cap != 0)
        assert text == m.describe_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16(*dims, scale or None, cap or None)
    for (T, G, MT), mp, cap in itertools.product(((1, 3, 1), (8, 4, 2), (2, 16, 2), (8, 1, 1)), (6, 256), (0.0, 50.0)):
        d = (3, T, 4 * G, 4, mp, 16, 256, 1000)
        rc, text = _describe(DEC + "_describe", *d, cap=cap)
        S, C, ws = plan_rule(3, T, 4 * G, 4, mp, 16, 1000)
        assert rc == len(text) > 0, (rc, text)
        assert text.startswith("fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_mfma<D=256,MT=%d,CAP=%d> softmax_scale=0.0625" % (MT, cap != 0))
        assert " S=%d C=%d " % (S, C) in text and "the 64-key steps" in text and "67072 bytes of static LDS" in text, text
        assert ("workspace %d bytes" % ws in text) == (S > 1) and (mp == 6) == (S == 1)
        assert text == m.describe_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(*d, None, cap or None)
    for mode, per_row in ((0, 32), (1, 16), (2, 32)):
        text = m.describe_kv_append_paged_varlen_d256_bf16(3, 40, 16, 8, 6, 16, 256, mode)
        assert text.startswith("kv_append_paged_varlen_bf16_rows<D=256,ROPE=%d>" % mode) and "%d threads per row" % per_row in text, text
        units = (2 * 8 + (16 if mode else 0)) * per_row
        assert "40 x %d workgroups" % ((units + 255) // 256) in text, text
    with pytest.raises(ValueError):
        m.describe_kv_append_paged_varlen_d256_bf16(3, 40, 16, 8, 6, 16, 128, 1)


# ---------------------------------------------------------------------------------------------------- the Python entries

def test_python_entries_refuse_bad_floats_and_forward_none(built, monkeypatch):
    from cuda_learn_notes_amd import host
    BF, i32 = torch.bfloat16, torch.int32
    ints = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32))
    b = lambda *s: torch.zeros(*s, dtype=BF)  # noqa: E731
    pb = lambda D=256: b(9, 2, 16, D)  # noqa: E731
    Hq = 8
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)
    monkeypatch.setattr(host, "_stream", lambda: None)
    seen = []
    monkeypatch.setattr(host, "_lse_fns", {n: (lambda n: lambda *a: seen.append((n, a)) or 0)(n) for n in (APP, PRE, DEC)})
    pre = lambda s, c, W=5, D=256: built.fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16(  # noqa: E731
        b(40, Hq, D), pb(D), pb(D), *ints, W, None, s, c, b(40, Hq, D))
    dec = lambda s, c, W=None, T=3, D=256: built.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(  # noqa: E731
        b(2, T, Hq, D), pb(D), pb(D), *ints[:2], W, None, s, c, b(2, T, Hq, D))
    for call in (pre, dec):
        for bad in BAD:
            with pytest.raises(RuntimeError, match=r"softmax_scale .* not supported \(finite and > 0, or None\)"):
                call(bad, None)
            with pytest.raises(RuntimeError, match=r"softcap .* not supported \(finite and > 0, or None\)"):
                call(None, bad)
        with pytest.raises(RuntimeError, match=r"head dim 128 not supported \(256\)"):
            call(None, None, D=128)
        with pytest.raises(RuntimeError, match=r"window 0 not supported"):
            call(None, None, W=0)
    with pytest.raises(RuntimeError, match=r"T 9 not supported \(1 … 8\)"):
        dec(None, None, T=9)
    assert not seen
    pre(None, 0), dec(0.0625, None), pre(None, 50.0, None), dec(None, 50, 7, 8)
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = seen
    assert (n0, n1, n2, n3) == (PRE, DEC, PRE, DEC)
    assert a0[-3:-1] == (0.0, 0.0) and a1[-3:-1] == (0.0625, 0.0) and a2[-3:-1] == (0.0, 50.0) and a3[-3:-1] == (0.0, 50.0)
    assert a0[-4] == 5 and a1[-4] == INT_MAX and a2[-4] == INT_MAX and a3[-4] == 7
    assert a0[6] is None and a1[5] is None  # sinks = None: a null pointer
    assert len(a0) == 21 and len(a1) == 22 and a0[-5] == 256 and a3[-5] == 256
    del seen[:]
    args = (b(40, 2, 256), b(40, 2, 256), pb(), pb(), *ints)
    built.kv_append_paged_varlen_d256_bf16(*args)
    built.kv_append_paged_varlen_d256_bf16(*args, b(40, Hq, 256), b(40, Hq, 256), torch.zeros(100, 256), "half")
    (n0, a0), (n1, a1) = seen
    assert n0 == n1 == APP and len(a0) == 21 and a0[7:10] == (None, None, None) and a0[-4:-1] == (256, 0, 0) and a1[-4:-1] == (256, 100, 1)
    with pytest.raises(RuntimeError, match=r"head dim 128 not supported \(256\)"):
        built.kv_append_paged_varlen_d256_bf16(b(40, 2, 128), b(40, 2, 128), pb(128), pb(128), *ints)
    with pytest.raises(RuntimeError, match=r"rope 'neox' not supported"):
        built.kv_append_paged_varlen_d256_bf16(*args, rope="neox")
    # the siblings keep their own texts
    with pytest.raises(RuntimeError, match=r"headdim 256 not supported \(64 or 128\)"):
        built.fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16(b(40, Hq, 256), pb(), pb(), *ints, 5, None, None, None, b(40, Hq, 256))


# ---------------------------------------------------------------------------------------------------- registers and instructions

def test_prefill_kernels_resources_and_mfma_count(tmp_path):
    """One workgroup per CU is what the kernel claims (__launch_bounds__(256, 1)): its LDS must fit 160 KB / 1. The loop's MFMAs: 4 key blocks x
    2 row tiles x 8 k-steps (D / 32) for S^T plus 2 halves of the step x 16 dim blocks (D / 16) x 2 row tiles for O^T = 64 + 64."""
    got = fs._bodies("flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16.hip", tmp_path)  # asserts no spill, no scratch
    assert len(got) == 2 and all("fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_mfma" in k["name"] for k, _ in got)
    rcps = {}
    for k, body in got:
        cap = "ILb1E" in k["name"]
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds")})
        assert k["lds"] == 2 * 64 * (2 * 256 + 32) and k["lds"] * 1 <= fs.LDS_PER_CU and k["vgpr"] <= 512, k
        assert fs._loop_mfmas(body) == 4 * 2 * (256 // 32) + 2 * (256 // 16) * 2 == 128, k["name"]
        assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]
        assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", ""), k["name"]
        rcps[cap] = body.count("v_rcp_f32")
    assert set(rcps) == {False, True}
    assert rcps[True] >= rcps[False] + 2 * 16, rcps  # the tanh: a v_rcp_f32 per score of a step's two row tiles (16 per lane and tile)


def test_decode_kernels_resources_mfma_counts_and_the_two_combines(tmp_path):
    """MT = 1 claims two workgroups per CU (__launch_bounds__(256, 2)), MT = 2 one. The loop's MFMAs per row tile: 8 k-steps (D / 32) of the
    wave's one 16-key block for S^T plus 16 dim blocks (D / 16) for O^T = 24 MT."""
    got = fs._bodies("flash_attn_decode_paged_multi_window_sink_softcap_anyg_d256_bf16.hip", tmp_path)  # asserts no spill, no scratch
    stream = [(k, b) for k, b in got if "fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_mfma" in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_window_" in k["name"]]
    assert len(stream) == 4 and len(combine) == 2 and len(got) == 6, [k["name"] for k, _ in got]
    rcps = {}
    for k, body in stream:
        m = re.search(r"ILi(\d)ELb(\d)E", k["name"])
        MT, cap = int(m.group(1)), m.group(2) == "1"
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds")})
        occupancy = 2 if MT == 1 else 1
        assert k["lds"] == 4 * 16 * (256 + 4 + 2) * 4 and k["lds"] * occupancy <= fs.LDS_PER_CU, k
        assert k["vgpr"] <= 512 // occupancy, k
        assert fs._loop_mfmas(body) == (256 // 32 + 256 // 16) * MT == 24 * MT, k["name"]
        assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]
        assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", ""), k["name"]
        rcps[(MT, cap)] = body.count("v_rcp_f32")
    assert set(rcps) == set(itertools.product((1, 2), (False, True)))
    for MT in (1, 2):  # the tanh: a v_rcp_f32 per score, 4 per lane and row tile, in the CAP kernels only
        assert rcps[(MT, True)] >= rcps[(MT, False)] + 4 * MT, rcps
    for k, body in combine:
        assert "ILi256E" in k["name"] and "v_cvt_pk_bf16_f32" in body and "global_store_short" in body and "v_mfma" not in body, k["name"]


def test_append_kernels_are_the_bf16_template_at_256(tmp_path):
    got = fs._bodies("kv_append_paged_varlen_d256_bf16.hip", tmp_path)  # asserts no spill, no scratch
    assert sorted(re.search(r"ILi(\d+)ELi(\d)E", k["name"]).groups() for k, _ in got) == [("256", "0"), ("256", "1"), ("256", "2")]
    for k, body in got:
        print(k["name"], {x: k.get(x) for x in ("vgpr", "sgpr", "lds")})
        assert "kv_append_paged_varlen_bf16_rows" in k["name"] and k["lds"] == 0 and "v_mfma" not in body
