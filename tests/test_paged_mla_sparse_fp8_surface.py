"""CPU: the sparse multi-head latent attention decode over the paged latent cache held in FP8 (include/cln_amd_ext.h:
cln_fa2_decode_paged_mla_sparse_bf16_fp8 with its plan and describe entries; csrc/flash_attn_decode_paged_mla_sparse_bf16_fp8.{cuh,hip}; DESIGN
4.4.23) -- the reference anchored to the two siblings' references, header, exports and package, the plan against the bf16 sparse entry's rule,
every status in its order (kv_scale and indices among the 4-byte inputs), the Python entry's refusals, the describe text against its manifest
mirror, the kernel's resources and instruction counts in the built library, and the condition under which the GPU parity cases can see where
kv_scale goes. No GPU needed: every refusal returns before a launch, and hipcc cross-compiles."""
import ctypes
import glob
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
import paged_mla_fp8_reference as mf  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import paged_mla_sparse_fp8_reference as s8  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of a code object)

DEC = "cln_fa2_decode_paged_mla_sparse_bf16_fp8"
NAMES = (DEC + "_plan", DEC, DEC + "_describe")
UNIT = "flash_attn_decode_paged_mla_sparse_bf16_fp8"
KERNEL = "fa2_decode_paged_mla_sparse_bf16_fp8_mfma"
BF, F8 = torch.bfloat16, mf.F8
NAN, INF = float("nan"), float("inf")
BAD_SCALES = (0.0, -1.0, NAN, INF, -INF)
LDS = 64 * (2 * 576 + 32)
P2 = 2.0 ** -8
DEC_ARGS = [ctypes.c_void_p] * 9 + [ctypes.c_longlong] + [ctypes.c_int] * 7 + [ctypes.c_float, ctypes.c_void_p]
_fn, _plan = fs._fn, fs._plan


def _describe(B, T, Hq, topk, max_pages, page, scale):
    fn = _fn(DEC + "_describe", [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(B, T, Hq, topk, max_pages, page, scale, buf, 4096)
    return rc, buf.value.decode()


# ---------------------------------------------------------------------------------------------------- the reference

def test_reference_is_the_bf16_sparse_one_on_the_dequantised_pool_at_a_power_of_two_scale():
    """kv_scale 2^-8: every product with it is exact, so O, LSE (to fp64 rounding) and the emulation (bit for bit) are
    paged_mla_sparse_reference.decode_sparse's on the pool dequantised to bf16, on random lists with empty slots of every kind."""
    T, Hq, page, topk = 3, 5, 16, 65
    q, lens, (pool, bt) = s8.one_case(T, Hq, page, P2)
    idx = s8.one_indices(T, Hq, page, topk).clone()
    idx[1, 0, :3] = torch.tensor([-7, 10 ** 6, lens[1]], dtype=torch.int32)
    o, l, e = s8.decode_sparse(q, pool, bt, lens, idx, P2, ml.SCALE)
    ro, rl, re_ = sp.decode_sparse(q, s8.deq_bf16(pool, bt, lens, P2), bt, lens, idx, ml.SCALE)
    fin = torch.isfinite(rl)
    assert bool(fin.any()) and not bool(fin.all()) and torch.equal(torch.isfinite(l), fin) and bool((l[~fin] == ml.NEG_INF).all())
    assert float((l[fin] - rl[fin]).abs().max()) < 1e-10 and float((o - ro).abs().max()) < 1e-12
    assert torch.equal(e, re_)


@pytest.mark.parametrize("kvs", s8.KV_SCALES, ids=["kv2^-8", "kv0.003"])
def test_reference_is_the_dense_fp8_one_on_the_dense_list(kvs):
    """indices[b, t] = [0 ... vis - 1, -1 ...]: O, LSE and the emulation are paged_mla_fp8_reference.decode's, tokens that see no key
    included; a mistake switched on in one is the same mistake in the other."""
    T, Hq, page = 3, 5, 16
    q, lens, (pool, bt) = s8.one_case(T, Hq, page, kvs)
    idx = sp.dense_indices(lens, T, sp.ONE_NMAX, sp.ONE_NMAX)
    for on in ((1, 1), (2, 1), (1, 0)):
        o, l, e = s8.decode_sparse(q, pool, bt, lens, idx, kvs, 0.11, *on)
        if on == (1, 1):
            ro, rl, _ = mf.decode(q, pool, bt, lens, kvs, 0.11)
            fin = torch.isfinite(rl)
            assert torch.equal(torch.isfinite(l), fin) and not bool(fin[0].any())
            assert float((l[fin] - rl[fin]).abs().max()) < 1e-10 and float((o - ro).abs().max()) < 1e-12
        assert torch.equal(e, mf.decode(q, pool, bt, lens, kvs, 0.11, ml.DC, *on)[2]), on


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_three_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    plan = "int, int, int, int, int, int, int*, int*, long long*"
    dec = ("const void*, const void*, const int*, const int*, const float*, const int*, void*, float*, void*, long long, " + "int, " * 7
           + "float, void*")
    dec_d = "int, int, int, int, int, int, float, char*, int"
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip((plan, dec, dec_d), NAMES)))
                   + "int main(void) { return f0 && f1 && f2 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_package_host_and_build_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_decode_paged_mla_sparse_bf16_fp8", "fa2_decode_paged_mla_sparse_bf16_fp8_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    assert hasattr(built.manifest, "describe_decode_paged_mla_sparse_bf16_fp8")
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    assert '"flash_attn_decode_paged_mla_sparse_bf16.hip", "%s.hip"' % UNIT in build  # behind the bf16 sparse unit
    assert all(os.path.exists(os.path.join(fs.CSRC, UNIT + e)) for e in (".hip", ".cuh"))
    # the three units share the two templates through one header and include no sibling's kernel header
    shared = "flash_attn_decode_paged_mla_shared.cuh"
    text = open(os.path.join(fs.CSRC, shared)).read()
    assert "store_split_scaled" in text and "fa2_decode_combine_bf16_all" in text and "__global__" in text and text.count("template <int D>") == 2
    for unit in (UNIT, "flash_attn_decode_paged_mla_sparse_bf16", "flash_attn_decode_paged_mla_bf16_fp8"):
        body = open(os.path.join(fs.CSRC, unit + ".cuh")).read().split("#pragma once")[1]
        assert '#include "%s"' % shared in body, unit
        assert not any('#include "%s.cuh"' % other in body for other in (UNIT, "flash_attn_decode_paged_mla_sparse_bf16",
                                                                           "flash_attn_decode_paged_mla_bf16_fp8", "flash_attn_decode_paged_mla_bf16"))


# ---------------------------------------------------------------------------------------------------- plan

def test_plan_is_the_bf16_sparse_entrys_rule(built):
    n = 0
    for B, (T, Hq), topk, (mp, page) in itertools.product((1, 5, 64, 1024), ((1, 1), (1, 64), (1, 65), (2, 128), (33, 16), (70, 5)),
                                                          (1, 63, 64, 65, 200, 256, 257, 2048, 5000, 100000), ((20, 16), (2048, 64))):
        got = _plan(DEC + "_plan", B, T, Hq, topk, mp, page)
        assert got == (0, sp.plan_rule(B, T, Hq, topk)) == _plan("cln_fa2_decode_paged_mla_sparse_bf16_plan", B, T, Hq, topk, mp, page)
        assert built.fa2_decode_paged_mla_sparse_bf16_fp8_plan(B, T, Hq, topk, mp, page) == got[1]
        n += 1
    assert n == 480
    for T, Hq in sp.SPLIT_TH:  # the GPU tests' shapes
        assert sp.plan_rule(5, T, Hq, 2048)[:2] == (8, 256)
    assert sp.plan_rule(5, 1, 16, 1024)[:2] == ml.plan_rule(5, 1, 16, 64, 16)[:2] == (4, 256)


def test_plan_refusals(built):
    p = lambda *dims: _plan(DEC + "_plan", *dims)[0]  # noqa: E731
    q = lambda *dims: _plan("cln_fa2_decode_paged_mla_sparse_bf16_plan", *dims)[0]  # noqa: E731
    for dims, want in (((1, 1, 16, 2048, 4, 16), 0), ((1, 70, 128, 1, 4, 16), 0), ((2, 1000, 1, 64, 4, 256), 0), ((1, 0, 16, 64, 4, 16), -1),
                       ((0, 1, 16, 64, 4, 16), -1), ((1, 1, 0, 64, 4, 16), -1), ((1, 1, 129, 64, 4, 16), -2), ((1, 1, 16, 0, 4, 16), -1),
                       ((1, 1, 16, -1, 4, 16), -1), ((1, 1, 16, 64, 4, 48), -2), ((1, 1, 16, 64, 4, 8), -2), ((1, 1, 16, 64, 1 << 23, 256), -2),
                       ((1, 1, 16, 64, (1 << 23) - 1, 256), 0), ((1, 1, 16, 64, 0, 16), -1), ((1, 1, 16, 64, 4, 0), -1),
                       ((1 << 20, 1 << 4, 128, 64, 4, 16), -2), ((1 << 16, 1 << 16, 1, 64, 4, 16), -2), ((1 << 20, 1 << 3, 128, 64, 4, 16), -2),
                       ((1 << 15, 1, 128, 64, 4, 16), 0)):
        assert p(*dims) == want == q(*dims), dims
    for args, text in (((1, 1, 129, 64, 4, 16), r"129 query heads not supported"), ((1, 1, 16, 64, 4, 48), r"page size 48 not supported"),
                       ((1 << 20, 1 << 4, 128, 64, 4, 16), r"too large for one launch"), ((1, 1, 16, 0, 4, 16), r"status -1")):
        with pytest.raises(RuntimeError, match=text):
            built.fa2_decode_paged_mla_sparse_bf16_fp8_plan(*args)


# ---------------------------------------------------------------------------------------------------- statuses of the entry

def test_every_status_in_its_order(built):
    """Scale, pointers (kv_scale and indices among the 4-byte aligned inputs, behind seqlens in that order), P, plan, workspace. Nothing is
    launched before a refusal."""
    fn = _fn(DEC, DEC_ARGS)
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    q, pool, bt, sl, ks, ix, o, lse, ws = (base + 256 * i for i in range(9))
    dims = (2, 1, 16, 64, 3, 4, 16)  # B, T, Hq, topk, P, max_pages, page: one split
    for bad in BAD_SCALES:
        assert fn(q, pool, bt, sl, ks, ix, o, lse, ws, 0, *dims, bad, None) == -1, bad
        assert fn(None, None, None, None, None, None, None, None, None, 0, 0, 0, 129, 0, 0, 0, 48, bad, None) == -1, bad  # before everything else
        assert _describe(2, 1, 16, 64, 4, 16, bad)[0] == -1, bad
    s = 192 ** -0.5
    call = lambda *a, d=dims, w=0: fn(*a, w, *d, s, None)  # noqa: E731
    ins = [q, pool, bt, sl, ks, ix, o]
    for i in range(7):  # a missing q, pool, table, lengths, kv_scale, indices or o -- ahead of an unsupported shape
        args = list(ins)
        args[i] = None
        assert call(*args, lse, ws) == -1 and call(*args, lse, ws, d=(2, 1, 129, 64, 3, 4, 16)) == -1, i
    for i, off in ((0, 8), (1, 8), (2, 2), (3, 2), (4, 2), (5, 2), (6, 8)):  # misaligned, one by one: 16 bytes, the 4-byte inputs 4
        args = list(ins)
        args[i] += off
        assert call(*args, lse, ws) == -1, i
    assert call(*ins, lse + 8, ws) == -1 and call(*ins, lse, ws + 8) == -1
    # 4-byte aligned inputs that are not 16-byte aligned pass the pointer check: the next refusal is P's
    odd = [q, pool, bt + 4, sl + 4, ks + 4, ix + 4, o]
    assert call(*odd, lse, ws, d=(2, 1, 16, 64, 0, 4, 16)) == -1
    assert call(*odd, lse, ws, d=(2, 1, 129, 64, 3, 4, 16)) == -2  # ... and with P the plan's, not -1
    for i in range(6):  # an output equal to an input, kv_scale and indices among them
        for out in range(3):
            args = [*ins, lse, ws]
            args[6 + out] = args[i]
            assert call(*args) == -1, (i, out)
    assert call(*ins, o, ws) == -1 and call(*ins, lse, lse) == -1  # ... or to another output
    assert call(*ins, None, None, d=(2, 1, 16, 64, 0, 4, 16)) == -1   # P, with lse and workspace absent
    assert call(*ins, lse, ws, d=(2, 1, 16, 64, 0, 4, 48)) == -1      # P before the plan
    assert call(*ins, lse, ws, d=(2, 1, 16, 0, 3, 4, 16)) == -1       # topk <= 0
    assert call(*ins, lse, ws, d=(2, 1, 16, -5, 3, 4, 16)) == -1
    assert call(*ins, lse, ws, d=(2, 1, 129, 64, 3, 4, 16)) == -2     # Hq = 129
    assert call(*ins, lse, ws, d=(2, 1, 16, 64, 3, 4, 48)) == -2      # the page
    assert call(*ins, lse, ws, d=(2, 0, 16, 64, 3, 4, 16)) == -1      # T = 0
    S, _, need = _plan(DEC + "_plan", 2, 1, 16, 2048, 4, 16)[1]
    assert S == 8 and need == 2 * 16 * S * 514 * 4
    assert call(*ins, lse, ws, d=(2, 1, 16, 2048, 3, 4, 16), w=need - 1) == -1  # a workspace too small for the splits
    assert call(*ins, lse, None, d=(2, 1, 16, 2048, 3, 4, 16), w=need) == -1
    assert call(*ins, lse, ws, d=(2, 1, 129, 2048, 3, 4, 16), w=0) == -2        # the plan before the workspace


# ---------------------------------------------------------------------------------------------------- describe text

def test_describe_text_equals_its_manifest_mirror(built):
    m = built.manifest
    s = 192 ** -0.5
    for B, T, Hq, topk, mp, page in ((64, 1, 16, 200, 256, 16), (5, 2, 40, 2048, 256, 16), (8, 1, 128, 2048, 2048, 64), (3, 70, 65, 1, 4, 16)):
        rc, text = _describe(B, T, Hq, topk, mp, page, s)
        S, C, ws = sp.plan_rule(B, T, Hq, topk)
        HG = -(-Hq // 64)
        assert rc == len(text) and text == m.describe_decode_paged_mla_sparse_bf16_fp8(B, T, Hq, topk, mp, page, s)
        assert text.startswith(KERNEL + "<Dk=576,Dv=512> ") and "v_mfma_f32_16x16x32_bf16" in text and "_f16" not in text
        s32 = float(torch.tensor(s, dtype=torch.float32))
        assert "softmax_scale=%.9g" % s32 in text
        assert "x log2(e) = %.9g times kv_scale (fp32 [1] on the device, read once per workgroup)" % float(torch.tensor(s32 * ml.LOG2E, dtype=torch.float32)) in text
        assert "T=%d Hq=%d topk=%d S=%d C=%d page=%d: %d workgroups" % (T, Hq, topk, S, C, page, B * T * HG * S) in text
        assert "(sequence, query token, group of 64 heads, split of C index slots; %d head groups)" % HG in text
        assert "index -> block table entry -> latent row of e4m3fn codes [c 512 | k_pe 64] (576 bytes)" in text and "9 16-byte loads per lane" in text
        assert "v_cvt_scalef32_pk_bf16_fp8, exact" in text and "72 MFMAs" in text and "64 MFMAs" in text
        assert "%d bytes static, row stride %d bytes" % (LDS, 2 * 576 + 32) in text
        assert "64 validity flags that travel in the pad bytes of LDS rows 0 and 1" in text and "a step without a valid slot skipped" in text
        assert "the fp32 result times kv_scale in front of its store" in text
        assert ("every split writes its partial, which carries kv_scale" in text and "workspace %d bytes" % ws in text
                and "fa2_decode_combine_bf16_all<D=512> merges all %d splits" % S in text) == (S > 1)
        assert (S > 1) == (topk == 2048) and text.endswith("; deterministic")
    for args, status in (((1, 1, 129, 64, 4, 16, s), -2), ((1, 1, 16, 0, 4, 16, s), -1), ((1, 1, 16, 64, 4, 16, 0.0), -1)):
        with pytest.raises(ValueError, match="status %d" % status):
            m.describe_decode_paged_mla_sparse_bf16_fp8(*args)


# ---------------------------------------------------------------------------------------------------- the Python entry

def test_python_entry_refuses_bad_tensors_before_any_device_call(built, monkeypatch):
    """No GPU: the device check is replaced, and a call that gets as far as the C entry shows it by raising Reached."""
    from cuda_learn_notes_amd import host

    class Reached(Exception):
        pass

    def reached(name, argtypes):
        raise Reached(name)

    devs = []
    monkeypatch.setattr(host, "_check_dev", lambda *ts: devs.append(ts))
    s = 192 ** -0.5
    b = lambda *sh: torch.zeros(*sh, dtype=BF)  # noqa: E731
    c8 = lambda *sh: torch.zeros(*sh, dtype=torch.uint8).view(F8)  # noqa: E731
    i = lambda *sh: torch.zeros(*sh, dtype=torch.int32)  # noqa: E731
    dec = built.fa2_decode_paged_mla_sparse_bf16_fp8
    good = dict(q=b(2, 3, 16, 576), pool=c8(3, 16, 576), block_table=i(2, 4), seqlens=i(2), kv_scale=torch.ones(1), indices=i(2, 3, 64),
                softmax_scale=s, out=b(2, 3, 16, 512))
    call = lambda **kw: dec(**{**good, **kw})  # noqa: E731
    for kw in (dict(q=good["q"].half()), dict(pool=b(3, 16, 576)), dict(pool=torch.zeros(3, 16, 576, dtype=torch.uint8)), dict(out=good["out"].half()),
               dict(seqlens=torch.zeros(2, dtype=torch.int64)), dict(indices=torch.zeros(2, 3, 64, dtype=torch.int64)),
               dict(block_table=torch.zeros(2, 4, dtype=torch.int64)), dict(lse=torch.zeros(2, 3, 16, dtype=torch.float64)),
               dict(kv_scale=torch.ones(1, dtype=torch.float64)), dict(kv_scale=torch.ones(1, dtype=BF))):
        with pytest.raises(RuntimeError, match="values must be"):
            call(**kw)
    devs.clear()
    with pytest.raises(RuntimeError, match="q of 575 dims not supported"):
        call(q=b(2, 3, 16, 575))
    # kv_scale went through the device check with the pool: a scale on another device is refused there
    assert any(any(t is good["kv_scale"] for t in ts) and any(t is good["pool"] for t in ts) for ts in devs)
    for kw in (dict(pool=c8(3, 16, 512)), dict(out=b(2, 3, 16, 576)), dict(lse=torch.zeros(2, 3, 15)), dict(q=b(2, 3, 576), out=b(2, 3, 512)),
               dict(indices=i(2, 64)), dict(indices=i(2, 3, 64, 1)), dict(indices=i(2, 2, 64)), dict(indices=i(3, 3, 64)), dict(seqlens=i(3)),
               dict(block_table=i(3, 4)), dict(pool=c8(48, 576)), dict(kv_scale=torch.ones(2)), dict(kv_scale=torch.ones(1, 1)),
               dict(kv_scale=torch.tensor(1.0))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            call(**kw)
    with pytest.raises(RuntimeError, match="indices must be contiguous"):
        call(indices=i(2, 3, 128)[:, :, ::2])
    with pytest.raises(RuntimeError, match="indices must be contiguous"):
        call(indices=i(3, 2, 64).transpose(0, 1))
    with pytest.raises((AttributeError, TypeError, RuntimeError)):
        call(kv_scale=None)  # a forgotten scale does not select the bf16 prototype
    with pytest.raises(TypeError):
        dec(good["q"], good["pool"], good["block_table"], good["seqlens"], good["indices"], s, good["out"])  # the bf16 entry's arguments
    for bad in BAD_SCALES:
        with pytest.raises(RuntimeError, match="softmax_scale .* not supported"):
            call(softmax_scale=bad)
    with pytest.raises(RuntimeError, match="129 query heads not supported"):
        call(q=b(2, 3, 129, 576), out=b(2, 3, 129, 512))
    with pytest.raises(RuntimeError, match="page size 48"):
        call(pool=c8(3, 48, 576))
    monkeypatch.setattr(host, "_ext_fn", reached)
    monkeypatch.setattr(host, "_decode_plan", lambda cname, dims: (0, (1, 64, 0)))
    with pytest.raises(Reached, match=DEC):
        call()
    with pytest.raises(Reached, match=DEC):  # T = 9 included
        call(q=b(2, 9, 16, 576), out=b(2, 9, 16, 512), indices=i(2, 9, 1), lse=torch.zeros(2, 9, 16))


def test_python_entry_refuses_a_kv_scale_on_another_device(built):
    """The real device check: everything on the CPU is refused as not being on the GPU before any device call."""
    b = lambda *sh: torch.zeros(*sh, dtype=BF)  # noqa: E731
    i = lambda *sh: torch.zeros(*sh, dtype=torch.int32)  # noqa: E731
    with pytest.raises(RuntimeError):
        built.fa2_decode_paged_mla_sparse_bf16_fp8(b(2, 3, 16, 576), torch.zeros(3, 16, 576, dtype=torch.uint8).view(F8), i(2, 4), i(2), torch.ones(1),
                                                   i(2, 3, 64), 0.07, b(2, 3, 16, 512))


# ---------------------------------------------------------------------------------------------------- registers and instructions

def _built_kernels(tmp_path):
    """{kernel name: metadata block} of the gfx950 code object of this unit inside the built product library."""
    from cuda_learn_notes_amd import _loader
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(objdump) and os.path.exists(readelf)
    local = str(tmp_path / "libcln_amd.so")
    shutil.copy(_loader.so_path("libcln_amd.so"), local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    out = {}
    for co in sorted(glob.glob(local + ".*gfx950")):
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
        if KERNEL not in notes:
            continue
        for blk in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, "- .agpr_count" + blk).group(1))
                         for k in ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                   "group_segment_fixed_size")}
    return out


def test_kernel_resources_in_the_built_library(built, tmp_path):
    """One workgroup per CU (__launch_bounds__(256, 1)): the unified file of 512 registers, no spill, no scratch, and the LDS the describe
    text states -- read from the code object inside the built library, which holds this kernel and its own instance of the combine."""
    got = _built_kernels(tmp_path)
    stream = [(n, k) for n, k in got.items() if KERNEL in n]
    combine = [(n, k) for n, k in got.items() if "fa2_decode_combine_bf16_all" in n]
    assert len(stream) == 1 and len(combine) == 1 and len(got) == 2, sorted(got)
    for n, k in stream + combine:
        print(n, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
    k = stream[0][1]
    assert 256 < k["vgpr_count"] <= 512 and k["agpr_count"] >= 128 and k["sgpr_count"] <= 102, k  # the 128 accumulators live in AGPRs
    assert k["group_segment_fixed_size"] == LDS == 75776 and LDS <= fs.LDS_PER_CU, k
    assert "%d bytes static" % k["group_segment_fixed_size"] in _describe(5, 2, 40, 2048, 256, 16, 0.07)[1]
    assert "ILi512E" in combine[0][0] and combine[0][1]["group_segment_fixed_size"] == 0


def test_kernel_instructions_are_the_join_of_the_siblings(tmp_path):
    """The loop's MFMAs per wave: 4 key blocks x 18 k-steps for S^T plus 32 dim blocks x 2 key pairs for O^T = 72 + 64 = 136, all bf16
    16x16x32, as in both siblings; 9 loads x 2 halves x 4 packed pairs = 72 v_cvt_scalef32_pk_bf16_fp8 in the kernel, as in the FP8 sibling; the
    flag byte store and the transposing reads of the sparse sibling; nothing through fp16 (fs._bodies asserts it, with no spill, no scratch)."""
    got = fs._bodies(UNIT + ".hip", tmp_path)
    for k, _ in got:
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds", "spill", "sgpr_spill", "scratch")})
    stream = [(k, b) for k, b in got if KERNEL in k["name"]]
    assert len(stream) == 1 and len(got) == 2, [k["name"] for k, _ in got]
    k, body = stream[0]
    assert k["lds"] == LDS and k["vgpr"] <= 512, k
    assert fs._loop_mfmas(body) == 4 * (576 // 32) + (512 // 16) * 2 == 136
    assert body.count("v_cvt_scalef32_pk_bf16_fp8") == 9 * 2 * 4 == 72
    assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body and "ds_write_b8" in body
    assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", "")
    sib = [fs._loop_mfmas(b) for u in ("flash_attn_decode_paged_mla_sparse_bf16.hip", "flash_attn_decode_paged_mla_bf16_fp8.hip")
           for kk, b in fs._bodies(u, tmp_path) if kk["name"].split("EPK")[0].endswith("_mfma")]
    assert sib == [136, 136], sib


# ---------------------------------------------------------------------------------------------------- the bound sees where kv_scale goes

def _margins(cases):
    worst = {}
    for what, q, lens, (pool, bt), idx, kvs in cases:
        for on, d, need in s8.margins(q, pool, bt, lens, idx, kvs):
            assert d >= need, (what, on, d, need)
            worst[on] = min(worst.get(on, INF), d / need)
    return worst


@pytest.mark.parametrize("kvs", s8.KV_SCALES, ids=["kv2^-8", "kv0.003"])
@pytest.mark.parametrize("TH", s8.ONE_TH, ids=lambda th: "T%dxHq%d" % th)
def test_the_one_split_parity_cases_would_notice_a_misplaced_kv_scale(TH, kvs):
    """On every one-split parity case of tests/test_gpu_paged_mla_sparse_fp8.py a reference with kv_scale dropped from the scores, twice in the
    scores, dropped from O or twice on O lies at least SENSITIVITY (20) x o_bound from the true one -- at topk 1, where one key has weight 1
    whatever its score, the two mistakes in the scores lie 20 x lse_tol from the true LSE instead. q x 128 (Q_MULT_ONE) is what it takes:
    paged_mla_sparse_fp8_reference records what each case needed."""
    worst = _margins(c for c in s8.parity_cases() if c[0][0] == "one" and c[0][1:3] == TH and c[-1] == kvs)
    print("mla sparse fp8 one split %s kv_scale %g: smallest distance / (20 x bound) per mistake %s" % (TH, kvs, {k: round(v, 2) for k, v in worst.items()}))


@pytest.mark.parametrize("kvs", s8.KV_SCALES, ids=["kv2^-8", "kv0.003"])
@pytest.mark.parametrize("TH", s8.SPLIT_TH, ids=lambda th: "T%dxHq%d" % th)
def test_the_several_splits_parity_cases_would_notice_a_misplaced_kv_scale(TH, kvs):
    """The same on the several-splits cases, q x 32 (Q_MULT_SPLIT)."""
    worst = _margins(c for c in s8.parity_cases() if c[0][0] == "split" and c[0][1:3] == TH and c[-1] == kvs)
    print("mla sparse fp8 several splits %s kv_scale %g: smallest distance / (20 x bound) per mistake %s" % (TH, kvs, {k: round(v, 2) for k, v in worst.items()}))


@pytest.mark.parametrize("scale", ml.OTHER_SCALES, ids=["yarn", "quarter"])
def test_the_gpu_case_at_another_scale_would_notice_the_datas_scale(scale):
    """tests/test_gpu_paged_mla_sparse_fp8.py runs scale_case(0.003) at V3's YaRN scale and at SCALE / 4: a kernel that ran at SCALE whatever
    it was given would be more than 20 x o_bound from the reference."""
    q, lens, (pool, bt), idx = s8.scale_case(0.003)
    ref, ref0 = s8.decode_sparse(q, pool, bt, lens, idx, 0.003, scale), s8.decode_sparse(q, pool, bt, lens, idx, 0.003, ml.SCALE, emul=False)
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla sparse fp8 scale %.5f: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, diff, need))
    assert diff > need
