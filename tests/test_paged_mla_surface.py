"""CPU: the multi-head latent attention entries over a paged latent cache (include/cln_amd_ext.h: cln_fa2_decode_paged_mla_bf16 with its plan
and describe entries, cln_kv_append_paged_mla_bf16 with its describe entry; csrc/*_mla_bf16.{cuh,hip}) -- the reference anchored
to the existing one, header, exports and package, the plan against a restatement of its rule, the refusals, the Python entries, the describe
texts and the kernels' resources. No GPU needed: hipcc cross-compiles."""
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
import paged_decode_reference as pr  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import paged_softcap_reference as cr  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of a code object)

DEC, APP = "cln_fa2_decode_paged_mla_bf16", "cln_kv_append_paged_mla_bf16"
NAMES = (DEC + "_plan", DEC, DEC + "_describe", APP, APP + "_describe")
BF = torch.bfloat16
NAN, INF = float("nan"), float("inf")
BAD_SCALES = (0.0, -1.0, NAN, INF, -INF)
_fn, _plan = fs._fn, fs._plan


def _describe_dec(B, T, Hq, max_pages, page, scale):
    fn = _fn(DEC + "_describe", [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(B, T, Hq, max_pages, page, scale, buf, 4096)
    return rc, buf.value.decode()


# ---------------------------------------------------------------------------------------------------- the reference

@pytest.mark.parametrize("D", [64, 128])
def test_reference_and_emulation_are_the_existing_ones_at_dv_equal_dk(D):
    """dv = dk = D and k_pages = v_pages = pool[:, None]: one KV head whose key and value are the same row. The fp64 O and LSE are
    paged_softcap_reference.decode's to rounding; the emulation is its emulation (that one rounds the fp64 P V sum to fp32 before the division,
    a step paged_bf16_reference.emul_rows does not have: at most one bf16 ulp apart, and equal in nearly every entry)."""
    g = torch.Generator().manual_seed(D)
    B, T, Hq, page, lens, scale = 3, 3, 5, 16, [40, 2, 0], 0.11
    q = torch.randn(B, T, Hq, D, generator=g).to(BF)
    dense = torch.randn(B, 48, D, generator=g).to(BF)
    pool, bt = ml.make_pool(dense, page, lens, seed=1)
    ro, rl, re_ = cr.decode(q, pool[:, None], pool[:, None], bt, lens, None, None, scale, None)
    o, l, e = ml.decode(q, pool, bt, lens, scale, dv=D)
    assert torch.equal(torch.isfinite(l), torch.isfinite(rl)) and bool((l[2] == ml.NEG_INF).all()) and bool((l[1, 0] == ml.NEG_INF).all())
    fin = torch.isfinite(rl)
    assert float((l[fin] - rl[fin]).abs().max()) < 1e-12 and float((o - ro).abs().max()) < 1e-12
    assert bool((e.bfloat16().double() == e).all())  # bf16 values
    diff = (e - re_).abs()
    assert float((diff / re_.abs().clamp(min=2.0 ** -126)).max()) <= 2.0 ** -7, "more than one bf16 ulp"
    assert float((diff != 0).double().mean()) < 0.01
    # and dv really is a parameter: the first dv dims of the value
    o2, l2, e2 = ml.decode(q, pool, bt, lens, scale, dv=D // 2)
    assert torch.equal(l2, l) and torch.equal(o2, o[..., :D // 2]) and torch.equal(e2, e[..., :D // 2])


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_five_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    plan = "int, int, int, int, int, int*, int*, long long*"
    dec = "const void*, const void*, const int*, const int*, void*, float*, void*, long long, " + "int, " * 6 + "float, void*"
    dec_d = "int, int, int, int, int, float, char*, int"
    app = "const void*, const void*, void*, const int*, const int*, const int*, const void*, void*, const float*, " + "int, " * 8 + "void*"
    app_d = "int, int, int, int, int, int, char*, int"
    protos = (plan, dec, dec_d, app, app_d)
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip(protos, NAMES)))
                   + "int main(void) { return f0 && f4 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_package_host_and_build_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_decode_paged_mla_bf16", "fa2_decode_paged_mla_bf16_plan", "kv_append_paged_mla_bf16"):
        assert hasattr(built, n) and hasattr(host, n), n
    m = built.manifest
    assert hasattr(m, "describe_decode_paged_mla_bf16") and hasattr(m, "describe_kv_append_paged_mla_bf16")
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    for unit in ("kv_append_paged_mla_bf16", "flash_attn_decode_paged_mla_bf16"):
        assert '"%s.hip"' % unit in build and os.path.exists(os.path.join(fs.CSRC, unit + ".hip")), unit
        assert os.path.exists(os.path.join(fs.CSRC, unit + ".cuh")), unit


# ---------------------------------------------------------------------------------------------------- plan

def test_plan_is_the_rule_restated(built):
    n = split = 0
    for B, (T, Hq), (mp, page) in itertools.product((1, 2, 5, 8, 64, 128, 1024),
                                                    ((1, 1), (1, 16), (1, 17), (3, 5), (1, 64), (5, 13), (2, 128), (8, 3), (2, 40), (1, 128), (8, 128)),
                                                    ((19, 16), (64, 16), (256, 16), (1024, 16), (64, 256), (100, 64), (256, 64), (16, 16))):
        got = _plan(DEC + "_plan", B, T, Hq, mp, page)
        want = ml.plan_rule(B, T, Hq, mp, page)
        assert got == (0, want), (B, T, Hq, mp, page, got, want)
        assert got[1][1] % max(page, ml.KEY_STEP) == 0 and got[1][0] * got[1][1] >= mp * page > (got[1][0] - 1) * got[1][1]
        assert built.fa2_decode_paged_mla_bf16_plan(B, T, Hq, mp, page) == got[1]
        n += 1
        split += got[1][0] > 1
    assert n > 500 and split > 100, (n, split)
    assert ml.plan_rule(5, 2, 40, 64, 16)[:2] == (4, 256)  # the GPU test's several-splits problem: B RG = 10


def test_plan_refusals(built):
    p = lambda *dims: _plan(DEC + "_plan", *dims)[0]  # noqa: E731
    assert p(1, 1, 16, 4, 16) == 0 and p(1, 8, 128, 4, 16) == 0
    assert p(1, 0, 16, 4, 16) == -1 and p(1, 9, 16, 4, 16) == -2          # T = 0 and 9
    assert p(1, 1, 0, 4, 16) == -1 and p(1, 1, 129, 4, 16) == -2          # Hq = 0 and 129
    assert p(1, 1, 16, 4, 48) == -2 and p(1, 1, 16, 4, 8) == -2 and p(1, 1, 16, 4, 512) == -2  # the page
    assert p(1, 1, 16, 1 << 23, 256) == -2 and p(1, 1, 16, (1 << 23) - 1, 256) == 0  # max_pages page past INT_MAX, and just inside
    assert p(0, 1, 16, 4, 16) == -1 and p(1, 1, 16, 0, 16) == -1 and p(1, 1, 16, 4, 0) == -1
    for args, text in (((1, 9, 16, 4, 16), r"T 9 not supported"), ((1, 1, 129, 4, 16), r"129 query heads not supported"),
                       ((1, 1, 16, 4, 48), r"page size 48 not supported"), ((1, 1, 16, 1 << 23, 256), r"too large for one launch"),
                       ((1, 0, 16, 4, 16), r"status -1")):
        with pytest.raises(RuntimeError, match=text):
            built.fa2_decode_paged_mla_bf16_plan(*args)


# ---------------------------------------------------------------------------------------------------- statuses of the entries

def test_scale_refusals_come_first_and_the_other_statuses_follow_the_siblings(built):
    fn = _fn(DEC, [ctypes.c_void_p] * 7 + [ctypes.c_longlong] + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_void_p])
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    q, pool, bt, sl, o, lse, ws = (base + 256 * i for i in range(7))
    dims = (2, 1, 16, 3, 4, 16)  # B, T, Hq, P, max_pages, page: one split, nothing is launched before a refusal
    for bad in BAD_SCALES:
        assert fn(q, pool, bt, sl, o, lse, ws, 0, *dims, bad, None) == -1, bad
        assert fn(None, None, None, None, None, None, None, 0, 0, 0, 0, 0, 0, 48, bad, None) == -1, bad  # before everything else
        assert _describe_dec(2, 1, 16, 4, 16, bad)[0] == -1, bad
    s = 192 ** -0.5
    for i in range(5):  # a missing q, pool, table, lengths or o
        args = [q, pool, bt, sl, o]
        args[i] = None
        assert fn(*args, lse, ws, 0, *dims, s, None) == -1, i
    assert fn(q + 8, pool, bt, sl, o, lse, ws, 0, *dims, s, None) == -1 and fn(q, pool, bt + 2, sl, o, lse, ws, 0, *dims, s, None) == -1  # alignment
    assert fn(q, pool, bt, sl, q, lse, ws, 0, *dims, s, None) == -1  # o is an input
    assert fn(q, pool, bt, sl, o, lse, ws, 0, 2, 1, 16, 0, 4, 16, s, None) == -1  # P
    assert fn(q, pool, bt, sl, o, lse, ws, 0, 2, 9, 16, 3, 4, 16, s, None) == -2 and fn(q, pool, bt, sl, o, lse, ws, 0, 2, 1, 16, 3, 4, 48, s, None) == -2
    S, _, need = _plan(DEC + "_plan", 2, 1, 16, 64, 16)[1]
    assert S > 1 and need == 2 * 16 * S * 514 * 4
    assert fn(q, pool, bt, sl, o, lse, ws, need - 1, 2, 1, 16, 3, 64, 16, s, None) == -1  # a workspace too small for the splits
    assert fn(q, pool, bt, sl, o, lse, None, need, 2, 1, 16, 3, 64, 16, s, None) == -1
    # the append: pointers, aliases, the rope arguments, the page
    ap = _fn(APP, [ctypes.c_void_p] * 9 + [ctypes.c_int] * 8 + [ctypes.c_void_p])
    c, kpe, pl, tb, ln, cu, qq, qo, rt = (base + 256 * i for i in range(9))
    ad = (2, 8, 16, 3, 4, 16)  # B, total_q, Hq, P, max_pages, page
    for i in range(6):
        args = [c, kpe, pl, tb, ln, cu]
        args[i] = None
        assert ap(*args, None, None, None, *ad, 0, 0, None) == -1, i
    assert ap(c, kpe, pl, tb, ln, cu, qq, None, None, *ad, 0, 0, None) == -1      # q without q_out
    assert ap(c, kpe, pl, tb, ln, cu, None, None, rt, *ad, 8, 0, None) == -1      # a table without a rotation
    assert ap(c, kpe, pl, tb, ln, cu, None, None, None, *ad, 8, 1, None) == -1    # a rotation without a table
    assert ap(c, kpe, pl, tb, ln, cu, None, None, rt, *ad, 0, 2, None) == -1      # ... without max_pos
    assert ap(c, kpe, c, tb, ln, cu, None, None, None, *ad, 0, 0, None) == -1     # the pool is an input
    assert ap(c, kpe, pl, tb, ln, cu, qq, pl, None, *ad, 0, 0, None) == -1        # q_out is the pool
    assert ap(c, kpe, pl, tb, ln, cu, None, None, None, 2, 8, 16, 3, 4, 48, 0, 0, None) == -2
    assert ap(c, kpe, pl, tb, ln, cu, None, None, None, 2, 0, 16, 3, 4, 16, 0, 0, None) == -1
    assert ap(c, kpe, pl, tb, ln, cu, None, None, None, 2, 8, 16, 3, 4, 16, 0, 3, None) == -2  # rope_mode 3


# ---------------------------------------------------------------------------------------------------- describe texts

def test_describe_texts_equal_their_manifest_mirrors(built):
    m = built.manifest
    s = 192 ** -0.5
    for B, T, Hq, mp, page in ((64, 1, 16, 256, 16), (5, 2, 40, 64, 16), (8, 2, 128, 256, 64), (3, 1, 1, 4, 16)):
        rc, text = _describe_dec(B, T, Hq, mp, page, s)
        S, C, ws = ml.plan_rule(B, T, Hq, mp, page)
        R = T * Hq
        assert rc == len(text) and text == m.describe_decode_paged_mla_bf16(B, T, Hq, mp, page, s)
        assert text.startswith("fa2_decode_paged_mla_bf16_mfma<Dk=576,Dv=512> ") and "v_mfma_f32_16x16x32_bf16" in text and "_f16" not in text
        assert "T=%d Hq=%d R=%d S=%d C=%d page=%d: %d workgroups" % (T, Hq, R, S, C, page, B * -(-R // 64) * S) in text
        assert "%d bytes static, row stride %d bytes" % (64 * (2 * 576 + 32), 2 * 576 + 32) in text
        assert ("fa2_decode_combine_bf16_rows<D=512>" in text and "workspace %d bytes" % ws in text) == (S > 1)
        assert text.endswith("; deterministic")
    with pytest.raises(ValueError, match="status -2"):
        m.describe_decode_paged_mla_bf16(1, 9, 16, 4, 16, s)
    with pytest.raises(ValueError, match="status -1"):
        m.describe_decode_paged_mla_bf16(1, 1, 16, 4, 16, 0.0)
    fn = _fn(APP + "_describe", [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_int])
    for mode, name in enumerate(("none", "half", "interleaved")):
        buf = ctypes.create_string_buffer(2048)
        rc = fn(5, 75, 16, 8, 16, mode, buf, 2048)
        text = buf.value.decode()
        assert rc == len(text) and text == m.describe_kv_append_paged_mla_bf16(5, 75, 16, 8, 16, name) == m.describe_kv_append_paged_mla_bf16(5, 75, 16, 8, 16, mode)
        ppr = 64 + (4 if mode == 1 else 8)
        assert text.startswith("kv_append_paged_mla_bf16_rows<ROPE=%d> " % mode) and "75 x %d workgroups" % -(-17 * ppr // 256) in text
        assert "%d threads per row" % ppr in text
    with pytest.raises(ValueError):
        m.describe_kv_append_paged_mla_bf16(5, 75, 16, 8, 48, 1)
    with pytest.raises(ValueError):
        m.describe_kv_append_paged_mla_bf16(5, 75, 16, 8, 16, "full")


# ---------------------------------------------------------------------------------------------------- the Python entries

def test_python_entries_refuse_bad_tensors_before_any_device_call(built, monkeypatch):
    """No GPU: the device check is replaced, and a call that gets as far as the C entry shows it by raising Reached."""
    from cuda_learn_notes_amd import host

    class Reached(Exception):
        pass

    def reached(name, argtypes):
        raise Reached(name)

    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)
    s = 192 ** -0.5
    b = lambda *sh: torch.zeros(*sh, dtype=BF)  # noqa: E731
    i = lambda *sh: torch.zeros(*sh, dtype=torch.int32)  # noqa: E731
    dec, app = built.fa2_decode_paged_mla_bf16, built.kv_append_paged_mla_bf16
    good = dict(q=b(2, 1, 16, 576), pool=b(3, 16, 576), block_table=i(2, 4), seqlens=i(2), softmax_scale=s, out=b(2, 1, 16, 512))
    call = lambda **kw: dec(**{**good, **kw})  # noqa: E731
    with pytest.raises(RuntimeError, match="values must be"):
        call(q=good["q"].half())
    with pytest.raises(RuntimeError, match="values must be"):
        call(pool=good["pool"].float())
    with pytest.raises(RuntimeError, match="values must be"):
        call(seqlens=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="values must be"):
        call(lse=torch.zeros(2, 1, 16, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="q of 575 dims not supported"):
        call(q=b(2, 1, 16, 575))
    with pytest.raises(RuntimeError, match="q of 512 dims not supported"):
        call(q=b(2, 1, 16, 512))
    with pytest.raises(RuntimeError, match="size mismatch"):
        call(pool=b(3, 16, 575))
    with pytest.raises(RuntimeError, match="size mismatch"):
        call(pool=b(3, 16, 512))
    with pytest.raises(RuntimeError, match="size mismatch"):
        call(out=b(2, 1, 16, 576))
    with pytest.raises(RuntimeError, match="size mismatch"):
        call(lse=torch.zeros(2, 1, 15))
    for bad in BAD_SCALES:
        with pytest.raises(RuntimeError, match="softmax_scale .* not supported"):
            call(softmax_scale=bad)
    with pytest.raises(TypeError):
        dec(good["q"], good["pool"], good["block_table"], good["seqlens"], None, good["out"])  # there is no default
    with pytest.raises(RuntimeError, match="T 9 not supported"):
        call(q=b(2, 9, 16, 576), out=b(2, 9, 16, 512))
    S, _, need = built.fa2_decode_paged_mla_bf16_plan(2, 1, 16, 64, 16)
    assert S > 1
    with pytest.raises(RuntimeError, match="workspace of %d bytes, the plan needs %d" % (need - 2, need)):
        call(block_table=i(2, 64), workspace=torch.zeros(need // 2 - 1, dtype=torch.int16))
    # the append
    ga = dict(c_new=b(8, 512), k_pe_new=b(8, 64), pool=b(3, 16, 576), block_table=i(2, 4), seqlens=i(2), cu_q=i(3))
    acall = lambda **kw: app(**{**ga, **kw})  # noqa: E731
    with pytest.raises(RuntimeError, match="values must be"):
        acall(c_new=ga["c_new"].half())
    with pytest.raises(RuntimeError, match="values must be"):
        acall(cu_q=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="size mismatch"):
        acall(c_new=b(8, 576))
    with pytest.raises(RuntimeError, match="size mismatch"):
        acall(k_pe_new=b(8, 32))
    with pytest.raises(RuntimeError, match="size mismatch"):
        acall(pool=b(3, 16, 512))
    with pytest.raises(RuntimeError, match="size mismatch"):
        acall(q=b(8, 4, 512), q_out=b(8, 4, 512))
    with pytest.raises(RuntimeError, match="size mismatch"):
        acall(cu_q=i(2))
    with pytest.raises(RuntimeError, match="size mismatch"):
        acall(q=b(8, 4, 576), q_out=b(8, 4, 576), rope_table=torch.zeros(64, 128), rope="half")
    with pytest.raises(RuntimeError, match="given together"):
        acall(q=b(8, 4, 576))
    with pytest.raises(RuntimeError, match="rope 'full' not supported"):
        acall(rope="full")
    with pytest.raises(RuntimeError, match="needs a rope_table"):
        acall(rope="half")
    with pytest.raises(RuntimeError, match="takes no rope_table"):
        acall(rope_table=torch.zeros(64, 64))
    with pytest.raises(RuntimeError, match="page size 48"):
        acall(pool=b(3, 48, 576))
    # a good call reaches the C entry
    monkeypatch.setattr(host, "_ext_fn", reached)
    monkeypatch.setattr(host, "_decode_plan", lambda cname, dims: (0, (1, 64, 0)))
    with pytest.raises(Reached, match=DEC):
        call()
    with pytest.raises(Reached, match=APP):
        acall(q=b(8, 4, 576), q_out=b(8, 4, 576), rope_table=torch.zeros(64, 64), rope="interleaved")


# ---------------------------------------------------------------------------------------------------- registers and instructions

def test_decode_kernel_resources_and_its_mfmas(tmp_path):
    """One workgroup per CU (__launch_bounds__(256, 1)): the unified file of 512 registers, one LDS image of 64 rows x 1184 bytes. The loop's
    MFMAs per wave: 4 key blocks x 18 k-steps for S^T plus 32 dim blocks x 2 key pairs for O^T = 72 + 64 = 136, all bf16 16x16x32."""
    got = fs._bodies("flash_attn_decode_paged_mla_bf16.hip", tmp_path)  # asserts no spill, no scratch
    for k, _ in got:
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds", "spill", "sgpr_spill", "scratch")})
    stream = [(k, b) for k, b in got if "fa2_decode_paged_mla_bf16_mfma" in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_bf16_rows" in k["name"]]
    assert len(stream) == 1 and len(combine) == 1 and len(got) == 2, [k["name"] for k, _ in got]
    k, body = stream[0]
    assert k["lds"] == 64 * (2 * 576 + 32) == 75776 and k["lds"] <= fs.LDS_PER_CU and k["vgpr"] <= 512, k
    assert fs._loop_mfmas(body) == 4 * (576 // 32) + (512 // 16) * 2 == 136
    assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body
    assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", "")
    k, body = combine[0]
    assert "ILi512E" in k["name"] and "v_cvt_pk_bf16_f32" in body and "v_mfma" not in body and k["lds"] == 0


def test_append_kernels_resources(tmp_path):
    got = fs._bodies("kv_append_paged_mla_bf16.hip", tmp_path)  # asserts no spill, no scratch
    assert sorted(re.search(r"rowsILi(\d)E", k["name"]).group(1) for k, _ in got) == ["0", "1", "2"]
    for k, body in got:
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds", "spill", "sgpr_spill", "scratch")})
        assert "kv_append_paged_mla_bf16_rows" in k["name"] and k["lds"] == 0 and "v_mfma" not in body


# ---------------------------------------------------------------------------------------------------- a scale that is not the data's

@pytest.mark.parametrize("scale", ml.OTHER_SCALES, ids=["yarn", "quarter"])
@pytest.mark.parametrize("case", ml.SCALE_TH, ids=lambda c: "T%dxHq%d%s" % (c[0], c[1], "-split" if c[2] else ""))
def test_the_gpu_cases_at_another_scale_would_notice_the_datas_scale(case, scale):
    """tests/test_gpu_paged_mla.py runs these cases at V3's YaRN scale and at SCALE / 4 with q x Q_MULT: a kernel that ran at SCALE whatever it
    was given would be more than 20 x o_bound from the reference."""
    assert abs(ml.YARN - 0.1353) < 1e-4 and ml.QUARTER == ml.SCALE / 4 and ml.Q_MULT & (ml.Q_MULT - 1) == 0
    ref, ref0 = ml.scale_case(*case, scale)[3:]
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla scale %.5f %s: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, case, diff, need))
    assert diff > need
