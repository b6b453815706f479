"""CPU: the multi-head latent attention entries over a paged latent cache held in FP8 (include/cln_amd_ext.h:
cln_fa2_decode_paged_mla_bf16_fp8 with its plan and describe entries, cln_kv_append_paged_mla_bf16_fp8 and cln_kv_gather_paged_mla_bf16_fp8 with
their describe entries; csrc/*_mla_bf16_fp8.{cuh,hip}) -- the reference anchored to the bf16 MLA reference, the parity cases of
the GPU file shown to be sensitive to a misplaced kv_scale and free of clamping, header, exports and package, the plan against the bf16 MLA
plan, the refusals in their order, the describe texts against their mirrors, the Python entries and the kernels' resources. No GPU needed:
hipcc cross-compiles."""
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
import fp8_kv_reference as f8  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_mla_fp8_reference as mf  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of a code object)

DEC, APP, GAT = "cln_fa2_decode_paged_mla_bf16_fp8", "cln_kv_append_paged_mla_bf16_fp8", "cln_kv_gather_paged_mla_bf16_fp8"
NAMES = (DEC + "_plan", DEC, DEC + "_describe", APP, APP + "_describe", GAT, GAT + "_describe")
SIB_PLAN = "cln_fa2_decode_paged_mla_bf16_plan"
BF, F8 = torch.bfloat16, f8.F8
NAN, INF = float("nan"), float("inf")
BAD_SCALES = (0.0, -1.0, NAN, INF, -INF)
SCALE = ml.SCALE
_fn, _plan = fs._fn, fs._plan
DEC_ARGS = [ctypes.c_void_p] * 8 + [ctypes.c_longlong] + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_void_p]
APP_ARGS = [ctypes.c_void_p] * 10 + [ctypes.c_int] * 8 + [ctypes.c_void_p]
GAT_ARGS = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 5 + [ctypes.c_void_p]


def _describe_dec(B, T, Hq, max_pages, page, scale):
    fn = _fn(DEC + "_describe", [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(B, T, Hq, max_pages, page, scale, buf, 4096)
    return rc, buf.value.decode()


# ---------------------------------------------------------------------------------------------------- the reference

def test_reference_and_emulation_are_the_bf16_mla_ones_at_a_power_of_two_scale():
    """kv_scale = 2^-8: dequantising to bf16 is exact, every product with the scale is exact, and the fp64 reference and the emulation ARE
    paged_mla_reference.decode's on the dequantised pool -- equal, not close. With 0.003 the fp64 reference still is that of the pool dequantised
    in float64 (by construction) and the emulation stays inside the family's distance of it."""
    g = torch.Generator().manual_seed(11)
    B, T, Hq, page, lens, kvs = 3, 3, 5, 16, [40, 2, 0], 2.0 ** -8
    q = (torch.randn(B, T, Hq, ml.DK, generator=g) * SCALE).to(BF)
    codes = mf.quantize((torch.randn(B, 48, ml.DK, generator=g) * SCALE).to(BF), kvs)
    pool, bt = mf.make_pool(codes, page, lens, seed=1)
    assert bool((f8.bits(pool[-1]) == f8.NAN_BYTE).all())  # the dead pages hold the NaN byte
    deq = mf.dequantize(mf.zero_dead_pages(pool, bt, lens), kvs).to(BF)
    assert torch.equal(deq.double(), mf.dequantize(mf.zero_dead_pages(pool, bt, lens), kvs, torch.float64))  # exact in bf16
    o, l, e = mf.decode(q, pool, bt, lens, kvs, SCALE)
    ro, rl, re_ = ml.decode(q, deq, bt, lens, SCALE)
    assert torch.equal(o, ro) and torch.equal(l, rl) and torch.equal(e, re_)
    assert bool((l[2] == ml.NEG_INF).all()) and bool((l[1, 0] == ml.NEG_INF).all()) and bool((e.bfloat16().double() == e).all())
    o3, l3, e3 = mf.decode(q, pool, bt, lens, 0.003, SCALE)
    fin = torch.isfinite(l3)
    assert torch.equal(fin, torch.isfinite(l)) and float((e3 - o3).abs().max()) <= 2.0 ** -7 * float(o3.abs().max())
    assert not torch.equal(o3, o)


def _away(ref, bound, o):
    return float((o - ref).abs().max()) / bound


def test_the_gpu_cases_would_notice_a_misplaced_kv_scale_and_never_clamp():
    """Every parity case of tests/test_gpu_paged_mla_fp8.py. Sensitivity, on the fp64 reference: kv_scale dropped from the scores (the scores of
    the codes: the reference at softmax_scale / kv_scale), dropped from O (O is linear in the values: O / kv_scale), and applied twice (the
    reference at softmax_scale kv_scale, times kv_scale) each lie more than 4 x the case's o_bound from the right O. No clamping: the inputs lie
    inside +-448 kv_scale and no code of a live row is +-448 or NaN."""
    worst = float("inf")
    for what, q, lens, (pool, bt), kvs in mf.parity_cases():
        dense = ml.gather(f8.bits(pool), bt, lens)
        live = torch.zeros(dense.shape[:2], dtype=torch.bool)
        for b, n in enumerate(lens):
            live[b, :n] = True
        c = dense[live]
        assert c.numel() and not bool(((c & 0x7F) >= 0x7E).any()), what  # neither +-448 (0x7e) nor NaN (0x7f)
        ro, _, emul = mf.decode(q, pool, bt, lens, kvs, SCALE)
        bound = br.o_bound(emul, ro)
        deq = mf.dequantize(mf.zero_dead_pages(pool, bt, lens), kvs, torch.float64)
        wrong = {"dropped on the scores": ml.decode(q, deq, bt, lens, SCALE / kvs)[0],
                 "dropped on O": ro / kvs,
                 "applied twice": ml.decode(q, deq, bt, lens, SCALE * kvs)[0] * kvs}
        for name, o in wrong.items():
            r = _away(ro, bound, o)
            assert r > 4, (what, name, r)
            worst = min(worst, r)
    for n, kvs in itertools.product((ml.ONE_NMAX, ml.SPLIT_PAGE * ml.SPLIT_MAX_PAGES), mf.KV_SCALES):
        x = ml._dense(len(ml.ONE_LENS) if n == ml.ONE_NMAX else len(ml.SPLIT_LENS), n)
        assert float(x.abs().max()) < f8.FP8_MAX * kvs
    print("smallest wrong / bound: %.1f" % worst)


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_seven_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    plan = "int, int, int, int, int, int*, int*, long long*"
    dec = "const void*, const void*, const int*, const int*, const float*, void*, float*, void*, long long, " + "int, " * 6 + "float, void*"
    dec_d = "int, int, int, int, int, float, char*, int"
    app = ("const void*, const void*, void*, const int*, const int*, const int*, const float*, const void*, void*, const float*, " + "int, " * 8
           + "void*")
    app_d = "int, int, int, int, int, int, char*, int"
    gat = "const void*, const int*, const int*, const int*, const float*, void*, " + "int, " * 5 + "void*"
    gat_d = "int, int, int, int, char*, int"
    protos = (plan, dec, dec_d, app, app_d, gat, gat_d)
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip(protos, NAMES)))
                   + "int main(void) { return f0 && f6 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_package_host_and_build_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_decode_paged_mla_bf16_fp8", "fa2_decode_paged_mla_bf16_fp8_plan", "kv_append_paged_mla_bf16_fp8", "kv_gather_paged_mla_bf16_fp8"):
        assert hasattr(built, n) and hasattr(host, n), n
    m = built.manifest
    for n in ("describe_decode_paged_mla_bf16_fp8", "describe_kv_append_paged_mla_bf16_fp8", "describe_kv_gather_paged_mla_bf16_fp8"):
        assert hasattr(m, n), n
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    for unit in ("kv_append_paged_mla_bf16_fp8", "flash_attn_decode_paged_mla_bf16_fp8", "kv_gather_paged_mla_bf16_fp8"):
        assert '"%s.hip"' % unit in build and os.path.exists(os.path.join(fs.CSRC, unit + ".hip")), unit
        assert os.path.exists(os.path.join(fs.CSRC, unit + ".cuh")), unit


# ---------------------------------------------------------------------------------------------------- plan

def test_plan_is_the_bf16_mla_plan_status_included(built):
    n = split = 0
    for B, (T, Hq), (mp, page) in itertools.product((1, 2, 5, 8, 64, 128, 1024),
                                                    ((1, 1), (1, 16), (1, 17), (3, 5), (1, 64), (5, 13), (2, 128), (8, 3), (2, 40), (1, 128), (8, 128)),
                                                    ((19, 16), (64, 16), (256, 16), (1024, 16), (64, 256), (100, 64), (256, 64), (16, 16))):
        got = _plan(DEC + "_plan", B, T, Hq, mp, page)
        assert got == _plan(SIB_PLAN, B, T, Hq, mp, page) == (0, ml.plan_rule(B, T, Hq, mp, page)), (B, T, Hq, mp, page, got)
        assert built.fa2_decode_paged_mla_bf16_fp8_plan(B, T, Hq, mp, page) == got[1]
        n += 1
        split += got[1][0] > 1
    assert n > 500 and split > 100, (n, split)
    for dims in ((1, 0, 16, 4, 16), (1, 9, 16, 4, 16), (1, 1, 0, 4, 16), (1, 1, 129, 4, 16), (1, 1, 16, 4, 48), (1, 1, 16, 4, 8), (1, 1, 16, 4, 512),
                 (1, 1, 16, 1 << 23, 256), (1, 1, 16, (1 << 23) - 1, 256), (0, 1, 16, 4, 16), (1, 1, 16, 0, 16), (1, 1, 16, 4, 0)):
        assert _plan(DEC + "_plan", *dims) == _plan(SIB_PLAN, *dims), dims  # the refusals, with the untouched out-parameters
    p = lambda *dims: _plan(DEC + "_plan", *dims)[0]  # noqa: E731
    assert p(1, 9, 16, 4, 16) == -2 and p(1, 0, 16, 4, 16) == -1 and p(1, 1, 129, 4, 16) == -2 and p(1, 1, 16, 4, 48) == -2
    for args, text in (((1, 9, 16, 4, 16), r"T 9 not supported"), ((1, 1, 129, 4, 16), r"129 query heads not supported"),
                       ((1, 1, 16, 4, 48), r"page size 48 not supported"), ((1, 1, 16, 1 << 23, 256), r"too large for one launch"),
                       ((1, 0, 16, 4, 16), r"status -1")):
        with pytest.raises(RuntimeError, match=text):
            built.fa2_decode_paged_mla_bf16_fp8_plan(*args)


# ---------------------------------------------------------------------------------------------------- statuses of the entries

def test_statuses_are_the_siblings_with_kv_scale_among_the_pointers(built):
    """Nothing is launched: every call below is refused. kv_scale stands behind seqlens (append: cu_q, gather: cu_k); a missing one, one that
    is not 4-byte aligned and one equal to an output are -1, before the shape (-2) is looked at."""
    fn = _fn(DEC, DEC_ARGS)
    buf = (ctypes.c_char * 8192)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    q, pool, bt, sl, kvs, o, lse, ws = (base + 256 * i for i in range(8))
    dims = (2, 1, 16, 3, 4, 16)  # B, T, Hq, P, max_pages, page: one split
    bad_shape = (2, 9, 16, 3, 4, 16)
    for bad in BAD_SCALES:
        assert fn(q, pool, bt, sl, kvs, o, lse, ws, 0, *dims, bad, None) == -1, bad
        assert fn(None, None, None, None, None, None, None, None, 0, 0, 0, 0, 0, 0, 48, bad, None) == -1, bad  # before everything else
        assert _describe_dec(2, 1, 16, 4, 16, bad)[0] == -1, bad
    s = SCALE
    for i in range(6):  # a missing q, pool, table, lengths, kv_scale or o
        args = [q, pool, bt, sl, kvs, o]
        args[i] = None
        assert fn(*args, lse, ws, 0, *bad_shape, s, None) == -1, i
    assert fn(q + 8, pool, bt, sl, kvs, o, lse, ws, 0, *dims, s, None) == -1 and fn(q, pool, bt + 2, sl, kvs, o, lse, ws, 0, *dims, s, None) == -1
    assert fn(q, pool, bt, sl, kvs + 2, o, lse, ws, 0, *bad_shape, s, None) == -1      # kv_scale misaligned, before the shape
    assert fn(q, pool, bt, sl, o, o, lse, ws, 0, *bad_shape, s, None) == -1            # kv_scale is o
    assert fn(q, pool, bt, sl, lse, o, lse, ws, 0, *bad_shape, s, None) == -1          # kv_scale is lse
    assert fn(q, pool, bt, sl, ws, o, lse, ws, 0, *bad_shape, s, None) == -1           # kv_scale is the workspace
    assert fn(q, pool, bt, sl, kvs, q, lse, ws, 0, *dims, s, None) == -1               # o is an input
    assert fn(q, pool, bt, sl, kvs, o, lse, ws, 0, 2, 1, 16, 0, 4, 16, s, None) == -1  # P
    assert fn(q, pool, bt, sl, kvs, o, lse, ws, 0, *bad_shape, s, None) == -2 and fn(q, pool, bt, sl, kvs, o, lse, ws, 0, 2, 1, 16, 3, 4, 48, s, None) == -2
    S, _, need = _plan(DEC + "_plan", 2, 1, 16, 64, 16)[1]
    assert S > 1 and need == 2 * 16 * S * 514 * 4
    assert fn(q, pool, bt, sl, kvs, o, lse, ws, need - 1, 2, 1, 16, 3, 64, 16, s, None) == -1  # a workspace too small for the splits
    assert fn(q, pool, bt, sl, kvs, o, lse, None, need, 2, 1, 16, 3, 64, 16, s, None) == -1
    # the append: pointers, aliases, the rope arguments, the page
    ap = _fn(APP, APP_ARGS)
    c, kpe, pl, tb, ln, cu, sc, qq, qo, rt = (base + 256 * i for i in range(10))
    ad = (2, 8, 16, 3, 4, 16)  # B, total_q, Hq, P, max_pages, page
    ad_bad = (2, 8, 16, 3, 4, 48)
    for i in range(7):
        args = [c, kpe, pl, tb, ln, cu, sc]
        args[i] = None
        assert ap(*args, None, None, None, *ad_bad, 0, 0, None) == -1, i
    assert ap(c, kpe, pl, tb, ln, cu, sc + 2, None, None, None, *ad_bad, 0, 0, None) == -1   # kv_scale misaligned, before the shape
    assert ap(c, kpe, pl, tb, ln, cu, pl, None, None, None, *ad_bad, 0, 0, None) == -1       # kv_scale is the pool
    assert ap(c, kpe, pl, tb, ln, cu, qo, qq, qo, None, *ad_bad, 0, 0, None) == -1           # kv_scale is q_out
    assert ap(c, kpe, pl, tb, ln, cu, sc, qq, None, None, *ad, 0, 0, None) == -1      # q without q_out
    assert ap(c, kpe, pl, tb, ln, cu, sc, None, None, rt, *ad, 8, 0, None) == -1      # a table without a rotation
    assert ap(c, kpe, pl, tb, ln, cu, sc, None, None, None, *ad, 8, 1, None) == -1    # a rotation without a table
    assert ap(c, kpe, pl, tb, ln, cu, sc, None, None, rt, *ad, 0, 2, None) == -1      # ... without max_pos
    assert ap(c, kpe, c, tb, ln, cu, sc, None, None, None, *ad, 0, 0, None) == -1     # the pool is an input
    assert ap(c, kpe, pl, tb, ln, cu, sc, qq, pl, None, *ad, 0, 0, None) == -1        # q_out is the pool
    assert ap(c, kpe, pl, tb, ln, cu, sc, None, None, None, *ad_bad, 0, 0, None) == -2
    assert ap(c, kpe, pl, tb, ln, cu, sc, None, None, None, 2, 0, 16, 3, 4, 16, 0, 0, None) == -1
    assert ap(c, kpe, pl, tb, ln, cu, sc, None, None, None, *ad, 0, 3, None) == -2    # rope_mode 3
    # the gather
    ga = _fn(GAT, GAT_ARGS)
    pl, tb, st, cu, sc, out = (base + 256 * i for i in range(6))
    gd, gd_bad = (2, 8, 3, 4, 16), (2, 8, 3, 4, 48)  # B, total_k, P, max_pages, page
    for i in (0, 1, 3, 4, 5):  # starts may be null
        args = [pl, tb, st, cu, sc, out]
        args[i] = None
        assert ga(*args, *gd_bad, None) == -1, i
    assert ga(pl, tb, st, cu, sc + 2, out, *gd_bad, None) == -1    # kv_scale misaligned, before the shape
    assert ga(pl, tb, st, cu, out, out, *gd_bad, None) == -1       # kv_scale is the output
    assert ga(pl, tb, st + 2, cu, sc, out, *gd, None) == -1 and ga(pl + 8, tb, st, cu, sc, out, *gd, None) == -1
    assert ga(pl, tb, st, cu, sc, pl, *gd, None) == -1             # the output is the pool
    assert ga(pl, tb, st, cu, sc, out, 2, 8, 0, 4, 16, None) == -1  # P
    assert ga(pl, tb, None, cu, sc, out, *gd_bad, None) == -2 and ga(pl, tb, st, cu, sc, out, 2, 0, 3, 4, 16, None) == -1


# ---------------------------------------------------------------------------------------------------- describe texts

def test_describe_texts_equal_their_manifest_mirrors(built):
    m = built.manifest
    s = SCALE
    for B, T, Hq, mp, page in ((64, 1, 16, 256, 16), (5, 2, 40, 64, 16), (8, 2, 128, 256, 64), (3, 1, 1, 4, 16)):
        rc, text = _describe_dec(B, T, Hq, mp, page, s)
        S, C, ws = ml.plan_rule(B, T, Hq, mp, page)
        R = T * Hq
        assert rc == len(text) and text == m.describe_decode_paged_mla_bf16_fp8(B, T, Hq, mp, page, s)
        assert text.startswith("fa2_decode_paged_mla_bf16_fp8_mfma<Dk=576,Dv=512> ") and "v_mfma_f32_16x16x32_bf16" in text and "_f16" not in text
        assert "(v_cvt_scalef32_pk_bf16_fp8, exact)" in text and "times kv_scale" in text
        assert "T=%d Hq=%d R=%d S=%d C=%d page=%d: %d workgroups" % (T, Hq, R, S, C, page, B * -(-R // 64) * S) in text
        assert "%d bytes static, row stride %d bytes" % (64 * (2 * 576 + 32), 2 * 576 + 32) in text and "75776 bytes static" in text
        assert ("fa2_decode_combine_bf16_rows<D=512>" in text and "workspace %d bytes" % ws in text) == (S > 1)
        assert text.endswith("; deterministic")
    with pytest.raises(ValueError, match="status -2"):
        m.describe_decode_paged_mla_bf16_fp8(1, 9, 16, 4, 16, s)
    with pytest.raises(ValueError, match="status -1"):
        m.describe_decode_paged_mla_bf16_fp8(1, 1, 16, 4, 16, 0.0)
    fn = _fn(APP + "_describe", [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_int])
    for mode, name in enumerate(("none", "half", "interleaved")):
        buf = ctypes.create_string_buffer(4096)
        rc = fn(5, 75, 16, 8, 16, mode, buf, 4096)
        text = buf.value.decode()
        assert rc == len(text) and text == m.describe_kv_append_paged_mla_bf16_fp8(5, 75, 16, 8, 16, name)
        assert text == m.describe_kv_append_paged_mla_bf16_fp8(5, 75, 16, 8, 16, mode)
        ppr = 64 + (4 if mode == 1 else 8)
        assert text.startswith("kv_append_paged_mla_bf16_fp8_rows<ROPE=%d> " % mode) and "75 x %d workgroups" % -(-17 * ppr // 256) in text
        assert "%d threads per row" % ppr in text and "(v_cvt_scalef32_pk_bf16_fp8, exact)" in text and "times kv_scale" in text
        assert text.endswith("; deterministic")
    with pytest.raises(ValueError):
        m.describe_kv_append_paged_mla_bf16_fp8(5, 75, 16, 8, 48, 1)
    with pytest.raises(ValueError):
        m.describe_kv_append_paged_mla_bf16_fp8(5, 75, 16, 8, 16, "full")
    rc, text = fs._describe(GAT + "_describe", 5, 75, 8, 16)
    assert rc == len(text) and text == m.describe_kv_gather_paged_mla_bf16_fp8(5, 75, 8, 16)
    assert text.startswith("kv_gather_paged_mla_bf16_fp8_rows B=5 total_k=75 page=16: ") and "75 x 1 workgroups" in text
    assert "(v_cvt_scalef32_pk_bf16_fp8, exact)" in text and "times kv_scale" in text and "= 128 written as zeros" in text
    with pytest.raises(ValueError):
        m.describe_kv_gather_paged_mla_bf16_fp8(5, 75, 8, 48)


# ---------------------------------------------------------------------------------------------------- the Python entries

def test_python_entries_refuse_bad_tensors_before_any_device_call(built, monkeypatch):
    """No GPU: the device check is replaced (one that refuses a marked tensor stands in for "on another device"), and a call that gets as far as
    the C entry shows it by raising Reached."""
    from cuda_learn_notes_amd import host

    class Reached(Exception):
        pass

    def reached(name, argtypes):
        raise Reached(name)

    elsewhere = torch.zeros(1, dtype=torch.float32)

    def check_dev(*ts):
        for t in ts:
            if t is elsewhere:
                raise RuntimeError("tensor on cuda:1 but the current device is cuda:0")

    monkeypatch.setattr(host, "_check_dev", check_dev)
    s = SCALE
    b = lambda *sh: torch.zeros(*sh, dtype=BF)  # noqa: E731
    c8 = lambda *sh: torch.zeros(*sh, dtype=torch.uint8).view(F8)  # noqa: E731
    i = lambda *sh: torch.zeros(*sh, dtype=torch.int32)  # noqa: E731
    kv = torch.ones(1, dtype=torch.float32)
    dec, app, gat = built.fa2_decode_paged_mla_bf16_fp8, built.kv_append_paged_mla_bf16_fp8, built.kv_gather_paged_mla_bf16_fp8
    good = dict(q=b(2, 1, 16, 576), pool=c8(3, 16, 576), block_table=i(2, 4), seqlens=i(2), kv_scale=kv, softmax_scale=s, out=b(2, 1, 16, 512))
    ga = dict(c_new=b(8, 512), k_pe_new=b(8, 64), pool=c8(3, 16, 576), block_table=i(2, 4), seqlens=i(2), cu_q=i(3), kv_scale=kv)
    gg = dict(pool=c8(3, 16, 576), block_table=i(2, 4), cu_k=i(3), kv_scale=kv, out=b(8, 576))
    call = lambda **kw: dec(**{**good, **kw})  # noqa: E731
    acall = lambda **kw: app(**{**ga, **kw})  # noqa: E731
    gcall = lambda **kw: gat(**{**gg, **kw})  # noqa: E731

    def refuses(f, text, **kw):
        with pytest.raises(RuntimeError, match=text) as e:
            f(**kw)
        assert not isinstance(e.value, Reached)

    for f in (call, acall, gcall):  # what the pool and its scale are asked
        refuses(f, "values must be torch::kFloat8_e4m3fn", pool=b(3, 16, 576))
        refuses(f, "values must be torch::kFloat8_e4m3fn", pool=torch.zeros(3, 16, 576, dtype=torch.uint8).view(torch.float8_e5m2))
        refuses(f, "values must be torch::kFloat32", kv_scale=torch.ones(1, dtype=torch.float64))
        refuses(f, "values must be torch::kFloat32", kv_scale=torch.ones(1, dtype=BF))
        refuses(f, "Tensor size mismatch!", kv_scale=torch.ones(2))
        refuses(f, "Tensor size mismatch!", kv_scale=torch.ones(()))
        refuses(f, "current device", kv_scale=elsewhere)
        refuses(f, "size mismatch", pool=c8(3, 16, 512))
        refuses(f, "size mismatch", pool=c8(3 * 16, 576))
    # the decode: what the sibling refuses
    refuses(call, "values must be", q=good["q"].half())
    refuses(call, "values must be", seqlens=torch.zeros(2, dtype=torch.int64))
    refuses(call, "values must be", out=good["out"].half())
    refuses(call, "values must be", lse=torch.zeros(2, 1, 16, dtype=torch.float64))
    refuses(call, "q of 575 dims not supported", q=b(2, 1, 16, 575))
    refuses(call, "size mismatch", out=b(2, 1, 16, 576))
    refuses(call, "size mismatch", lse=torch.zeros(2, 1, 15))
    for bad in BAD_SCALES:
        refuses(call, "softmax_scale .* not supported", softmax_scale=bad)
    with pytest.raises(TypeError):
        dec(good["q"], good["pool"], good["block_table"], good["seqlens"], kv, None, good["out"])  # there is no default
    refuses(call, "T 9 not supported", q=b(2, 9, 16, 576), out=b(2, 9, 16, 512))
    S, _, need = built.fa2_decode_paged_mla_bf16_fp8_plan(2, 1, 16, 64, 16)
    assert S > 1
    refuses(call, "workspace of %d bytes, the plan needs %d" % (need - 2, need), block_table=i(2, 64),
            workspace=torch.zeros(need // 2 - 1, dtype=torch.int16))
    # the append
    refuses(acall, "values must be", c_new=ga["c_new"].half())
    refuses(acall, "values must be", cu_q=torch.zeros(3, dtype=torch.int64))
    refuses(acall, "size mismatch", c_new=b(8, 576))
    refuses(acall, "size mismatch", k_pe_new=b(8, 32))
    refuses(acall, "size mismatch", q=b(8, 4, 512), q_out=b(8, 4, 512))
    refuses(acall, "size mismatch", cu_q=i(2))
    refuses(acall, "size mismatch", q=b(8, 4, 576), q_out=b(8, 4, 576), rope_table=torch.zeros(64, 128), rope="half")
    refuses(acall, "given together", q=b(8, 4, 576))
    refuses(acall, "rope 'full' not supported", rope="full")
    refuses(acall, "needs a rope_table", rope="half")
    refuses(acall, "takes no rope_table", rope_table=torch.zeros(64, 64))
    refuses(acall, "page size 48", pool=c8(3, 48, 576))
    # the gather
    refuses(gcall, "values must be", out=b(8, 576).half())
    refuses(gcall, "values must be", starts=torch.zeros(2, dtype=torch.int64))
    refuses(gcall, "size mismatch", out=b(8, 512))
    refuses(gcall, "size mismatch", cu_k=i(2))
    refuses(gcall, "size mismatch", starts=i(3))
    refuses(gcall, "page size 48", pool=c8(3, 48, 576))
    # a good call reaches the C entry
    monkeypatch.setattr(host, "_ext_fn", reached)
    monkeypatch.setattr(host, "_decode_plan", lambda cname, dims: (0, (1, 64, 0)))
    with pytest.raises(Reached, match=DEC):
        call()
    with pytest.raises(Reached, match=APP):
        acall(q=b(8, 4, 576), q_out=b(8, 4, 576), rope_table=torch.zeros(64, 64), rope="interleaved")
    with pytest.raises(Reached, match=GAT):
        gcall(starts=i(2))


# ---------------------------------------------------------------------------------------------------- registers and instructions

def _resources(k):
    return {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds", "spill", "sgpr_spill", "scratch")}


def test_decode_kernel_resources_its_mfmas_and_its_conversions(tmp_path):
    """One workgroup per CU (__launch_bounds__(256, 1)): the unified file of 512 registers, the sibling's one LDS image of 64 rows x 1184 bytes.
    The loop's MFMAs per wave are the sibling's: 72 for S^T plus 64 for O^T = 136, all bf16 16x16x32. The loop converts 9 x 16 codes per lane:
    72 packed conversions. No spill, no scratch, no _f16 instruction (fs._bodies)."""
    got = fs._bodies("flash_attn_decode_paged_mla_bf16_fp8.hip", tmp_path)  # asserts no spill, no scratch, no _f16
    for k, _ in got:
        print(k["name"], _resources(k))
    stream = [(k, b) for k, b in got if "fa2_decode_paged_mla_bf16_fp8_mfma" in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_bf16_rows" in k["name"]]
    assert len(stream) == 1 and len(combine) == 1 and len(got) == 2, [k["name"] for k, _ in got]
    k, body = stream[0]
    assert k["lds"] == 64 * (2 * 576 + 32) == 75776 and k["lds"] <= fs.LDS_PER_CU and k["vgpr"] <= 512, k
    assert fs._loop_mfmas(body) == 4 * (576 // 32) + (512 // 16) * 2 == 72 + 64
    assert body.count("v_cvt_scalef32_pk_bf16_fp8") == 9 * 8 == 72
    assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body and "global_load_dwordx4" in body
    assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", "")
    sib = [(ks, b) for ks, b in fs._bodies("flash_attn_decode_paged_mla_bf16.hip", tmp_path) if "_mfma" in ks["name"]]
    assert len(sib) == 1 and fs._loop_mfmas(sib[0][1]) == fs._loop_mfmas(body) and sib[0][0]["lds"] == k["lds"]
    k, body = combine[0]
    assert "ILi512E" in k["name"] and "v_cvt_pk_bf16_f32" in body and "v_mfma" not in body and k["lds"] == 0


def test_append_and_gather_kernels_resources(tmp_path):
    got = fs._bodies("kv_append_paged_mla_bf16_fp8.hip", tmp_path)  # asserts no spill, no scratch, no _f16
    assert sorted(re.search(r"rowsILi(\d)E", k["name"]).group(1) for k, _ in got) == ["0", "1", "2"]
    for k, body in got:
        print(k["name"], _resources(k))
        assert "kv_append_paged_mla_bf16_fp8_rows" in k["name"] and k["lds"] == 0 and "v_mfma" not in body and k["vgpr"] <= 512
        assert "v_cvt_pk_fp8_f32" in body
    got = fs._bodies("kv_gather_paged_mla_bf16_fp8.hip", tmp_path)
    assert len(got) == 1
    k, body = got[0]
    print(k["name"], _resources(k))
    assert "kv_gather_paged_mla_bf16_fp8_rows" in k["name"] and k["lds"] == 0 and "v_mfma" not in body and k["vgpr"] <= 512
    assert body.count("v_cvt_scalef32_pk_bf16_fp8") == 4 and "v_cvt_pk_bf16_f32" in body


# ---------------------------------------------------------------------------------------------------- a scale that is not the data's

@pytest.mark.parametrize("kvs", mf.KV_SCALES, ids=["kv2^-8", "kv0.003"])
@pytest.mark.parametrize("scale", ml.OTHER_SCALES, ids=["yarn", "quarter"])
@pytest.mark.parametrize("case", ml.SCALE_TH, ids=lambda c: "T%dxHq%d%s" % (c[0], c[1], "-split" if c[2] else ""))
def test_the_gpu_cases_at_another_scale_would_notice_the_datas_scale(case, scale, kvs):
    """tests/test_gpu_paged_mla_fp8.py runs these cases at V3's YaRN scale and at SCALE / 4 with q x Q_MULT: a kernel whose scale_log2 kv_scale
    product held SCALE whatever it was given would be more than 20 x o_bound from the reference."""
    ref, ref0 = mf.scale_case(*case, kvs, scale)[3:]
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla fp8 scale %.5f kv_scale %g %s: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, kvs, case, diff, need))
    assert diff > need
