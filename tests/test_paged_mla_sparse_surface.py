"""CPU: the sparse multi-head latent attention decode over the paged latent cache (include/cln_amd_ext.h:
cln_fa2_decode_paged_mla_sparse_bf16 with its plan and describe entries; csrc/flash_attn_decode_paged_mla_sparse_bf16.{cuh,hip}; DESIGN
4.4.20) -- the reference anchored to paged_mla_reference.decode, header, exports and package, the plan against a restatement of its rule, every
status in its order, the Python entries' refusals, the describe text against its manifest mirror and the kernel's resources in the built
library. No GPU needed: every refusal returns before a launch, and hipcc cross-compiles."""
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
import paged_mla_reference as ml  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of a code object)

DEC = "cln_fa2_decode_paged_mla_sparse_bf16"
NAMES = (DEC + "_plan", DEC, DEC + "_describe")
UNIT = "flash_attn_decode_paged_mla_sparse_bf16"
BF = torch.bfloat16
NAN, INF = float("nan"), float("inf")
BAD_SCALES = (0.0, -1.0, NAN, INF, -INF)
LDS = 64 * (2 * 576 + 32)
DEC_ARGS = [ctypes.c_void_p] * 8 + [ctypes.c_longlong] + [ctypes.c_int] * 7 + [ctypes.c_float, ctypes.c_void_p]
_fn, _plan = fs._fn, fs._plan


def _describe(B, T, Hq, topk, max_pages, page, scale):
    fn = _fn(DEC + "_describe", [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(B, T, Hq, topk, max_pages, page, scale, buf, 4096)
    return rc, buf.value.decode()


# ---------------------------------------------------------------------------------------------------- the reference

def test_reference_is_the_dense_one_on_the_dense_list_and_ignores_the_order():
    """indices[b, t] = [0 ... vis - 1, -1 ...]: O, LSE and the emulation are paged_mla_reference.decode's on the same inputs (lengths below T
    included: tokens that see no key). A permuted list with the empty slots scattered gives the same fp64 result to rounding."""
    g = torch.Generator().manual_seed(3)
    B, T, Hq, page, lens, scale, topk = 4, 3, 5, 16, [40, 2, 0, 48], 0.11, 64
    q = torch.randn(B, T, Hq, ml.DK, generator=g).to(BF)
    pool, bt = ml.make_pool(torch.randn(B, 48, ml.DK, generator=g).to(BF), page, lens, seed=1)
    idx = sp.dense_indices(lens, T, 48, topk)
    assert idx[0, 2].tolist() == list(range(40)) + [-1] * 24 and idx[1, 0].tolist() == [-1] * 64 and idx[1, 1].tolist() == [0] + [-1] * 63
    o, l, e = sp.decode_sparse(q, pool, bt, lens, idx, scale)
    ro, rl, re_ = ml.decode(q, pool, bt, lens, scale)
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(l), fin) and bool((l[~fin] == ml.NEG_INF).all()) and not bool(fin[2].any()) and not bool(fin[1, 0].any())
    assert float((l[fin] - rl[fin]).abs().max()) < 1e-12 and float((o - ro).abs().max()) < 1e-12
    assert torch.equal(e, re_)  # the emulation is emul_rows on the same rows in the same order
    perm = idx.clone()
    for b in range(B):
        for t in range(T):
            perm[b, t] = idx[b, t][torch.randperm(topk, generator=g)]
    assert not torch.equal(perm, idx)
    po, pl_, _ = sp.decode_sparse(q, pool, bt, lens, perm, scale)
    assert float((po - o).abs().max()) < 1e-12 and float((pl_[fin] - l[fin]).abs().max()) < 1e-12
    # every kind of empty slot is empty, and a duplicate is two keys
    odd = idx.clone()
    odd[0, 2, 40:46] = torch.tensor([-7, 40, 41, 47, 53, 2 ** 31 - 1], dtype=torch.int32)  # vis = 40 itself, len + 1, Nmax - 1, past the cache
    assert all(torch.equal(a, b) for a, b in zip(sp.decode_sparse(q, pool, bt, lens, odd, scale), (o, l, e)))
    dup = idx.clone()
    dup[0, 2, 40] = 7
    dl = sp.decode_sparse(q, pool, bt, lens, dup, scale)[1]
    want = torch.logaddexp(l[0, 2], q[0, 2].double() @ pool[int(bt[0, 0]), 7].double() * sp.cr.f32(scale))  # key 7 once more
    assert float((dl[0, 2] - want).abs().max()) < 1e-12 and bool((dl[0, 2] > l[0, 2]).all())


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_three_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    plan = "int, int, int, int, int, int, int*, int*, long long*"
    dec = "const void*, const void*, const int*, const int*, const int*, void*, float*, void*, long long, " + "int, " * 7 + "float, void*"
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
    for n in ("fa2_decode_paged_mla_sparse_bf16", "fa2_decode_paged_mla_sparse_bf16_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    assert hasattr(built.manifest, "describe_decode_paged_mla_sparse_bf16")
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    assert '"%s.hip"' % UNIT in build and all(os.path.exists(os.path.join(fs.CSRC, UNIT + e)) for e in (".hip", ".cuh"))
    assert "flash_attn_decode_paged_mla_bf16.cuh" not in open(os.path.join(fs.CSRC, UNIT + ".cuh")).read().split("#pragma once")[1]


# ---------------------------------------------------------------------------------------------------- plan

def test_plan_is_the_rule_restated(built):
    n = split = 0
    for B, (T, Hq), topk, (mp, page) in itertools.product((1, 2, 5, 8, 64, 1024), ((1, 1), (1, 16), (1, 64), (1, 65), (2, 128), (8, 3), (33, 16), (70, 5)),
                                                          (1, 63, 64, 65, 200, 256, 257, 1000, 2048, 5000, 100000), ((20, 16), (256, 16), (2048, 64))):
        got = _plan(DEC + "_plan", B, T, Hq, topk, mp, page)
        want = sp.plan_rule(B, T, Hq, topk)
        assert got == (0, want), (B, T, Hq, topk, mp, page, got, want)
        S, C, _ = got[1]
        assert C % 64 == 0 and S * C >= topk > (S - 1) * C and S <= 64
        assert built.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, topk, mp, page) == got[1]
        n += 1
        split += S > 1
    assert n > 1000 and split > 200, (n, split)
    # the GPU test's shapes: 8 splits of 256 slots at topk 2048 and B = 5; the dense entry's plan at Nmax = topk = 1024, T = 1
    for T, Hq in sp.SPLIT_TH:
        assert sp.plan_rule(5, T, Hq, 2048)[:2] == (8, 256)
    for Hq in (16, 128):
        assert sp.plan_rule(5, 1, Hq, 1024)[:2] == ml.plan_rule(5, 1, Hq, 64, 16)[:2] == (4, 256)
    for T, Hq in sp.ONE_TH:
        assert sp.plan_rule(8, T, Hq, 320)[0] == ml.plan_rule(8, T, Hq, 20, 16)[0] == 1


def test_plan_refusals(built):
    p = lambda *dims: _plan(DEC + "_plan", *dims)[0]  # noqa: E731
    assert p(1, 1, 16, 2048, 4, 16) == 0 and p(1, 70, 128, 1, 4, 16) == 0 and p(2, 1000, 1, 64, 4, 256) == 0  # T has no cap
    assert p(1, 0, 16, 64, 4, 16) == -1 and p(0, 1, 16, 64, 4, 16) == -1
    assert p(1, 1, 0, 64, 4, 16) == -1 and p(1, 1, 129, 64, 4, 16) == -2          # Hq = 0 and 129
    assert p(1, 1, 16, 0, 4, 16) == -1 and p(1, 1, 16, -1, 4, 16) == -1          # topk <= 0
    assert p(1, 1, 16, 64, 4, 48) == -2 and p(1, 1, 16, 64, 4, 8) == -2 and p(1, 1, 16, 64, 4, 512) == -2  # the page
    assert p(1, 1, 16, 64, 1 << 23, 256) == -2 and p(1, 1, 16, 64, (1 << 23) - 1, 256) == 0  # max_pages page past INT_MAX, and just inside
    assert p(1, 1, 16, 64, 0, 16) == -1 and p(1, 1, 16, 64, 4, 0) == -1
    assert p(1 << 20, 1 << 4, 128, 64, 4, 16) == -2 and p(1 << 16, 1 << 16, 1, 64, 4, 16) == -2  # B T Hq and B T past an int
    assert p(1 << 20, 1 << 3, 128, 64, 4, 16) == -2 and p(1 << 15, 1, 128, 64, 4, 16) == 0     # rows fit an int, the grid does not; and both do
    for args, text in (((1, 1, 129, 64, 4, 16), r"129 query heads not supported"), ((1, 1, 16, 64, 4, 48), r"page size 48 not supported"),
                       ((1 << 20, 1 << 4, 128, 64, 4, 16), r"too large for one launch"), ((1, 1, 16, 0, 4, 16), r"status -1")):
        with pytest.raises(RuntimeError, match=text):
            built.fa2_decode_paged_mla_sparse_bf16_plan(*args)


# ---------------------------------------------------------------------------------------------------- statuses of the entry

def test_every_status_in_its_order(built):
    """Scale, pointers (indices among the 4-byte aligned int inputs), P, plan, workspace. Nothing is launched before a refusal."""
    fn = _fn(DEC, DEC_ARGS)
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    q, pool, bt, sl, ix, o, lse, ws = (base + 256 * i for i in range(8))
    dims = (2, 1, 16, 64, 3, 4, 16)  # B, T, Hq, topk, P, max_pages, page: one split
    for bad in BAD_SCALES:
        assert fn(q, pool, bt, sl, ix, o, lse, ws, 0, *dims, bad, None) == -1, bad
        assert fn(None, None, None, None, None, None, None, None, 0, 0, 0, 129, 0, 0, 0, 48, bad, None) == -1, bad  # before everything else
        assert _describe(2, 1, 16, 64, 4, 16, bad)[0] == -1, bad
    s = 192 ** -0.5
    call = lambda *a, d=dims, w=0: fn(*a, w, *d, s, None)  # noqa: E731
    for i in range(6):  # a missing q, pool, table, lengths, indices or o -- ahead of an unsupported shape
        args = [q, pool, bt, sl, ix, o]
        args[i] = None
        assert call(*args, lse, ws) == -1 and call(*args, lse, ws, d=(2, 1, 129, 64, 3, 4, 16)) == -1, i
    for i, off in ((0, 8), (1, 8), (2, 2), (3, 2), (4, 2), (5, 8)):  # misaligned, one by one: 16 bytes, the int inputs 4
        args = [q, pool, bt, sl, ix, o]
        args[i] += off
        assert call(*args, lse, ws) == -1, i
    assert call(q, pool, bt, sl, ix, o, lse + 8, ws) == -1 and call(q, pool, bt, sl, ix, o, lse, ws + 8) == -1
    # 4-byte aligned int inputs that are not 16-byte aligned pass the pointer check: the next refusal is P's
    assert call(q, pool, bt + 4, sl + 4, ix + 4, o, lse, ws, d=(2, 1, 16, 64, 0, 4, 16)) == -1
    assert call(q, pool, bt + 4, sl + 4, ix + 4, o, lse, ws, d=(2, 1, 129, 64, 3, 4, 16)) == -2  # ... and with P the plan's, not -1
    for i in range(5):  # an output equal to an input
        for out in range(3):
            args = [q, pool, bt, sl, ix, o, lse, ws]
            args[5 + out] = args[i]
            assert call(*args) == -1, (i, out)
    assert call(q, pool, bt, sl, ix, o, o, ws) == -1 and call(q, pool, bt, sl, ix, o, lse, lse) == -1  # ... or to another output
    assert call(q, pool, bt, sl, ix, o, None, None, d=(2, 1, 16, 64, 0, 4, 16)) == -1  # P, with lse and workspace absent
    assert call(q, pool, bt, sl, ix, o, lse, ws, d=(2, 1, 16, 64, 0, 4, 48)) == -1     # P before the plan
    assert call(q, pool, bt, sl, ix, o, lse, ws, d=(2, 1, 16, 0, 3, 4, 16)) == -1      # topk <= 0
    assert call(q, pool, bt, sl, ix, o, lse, ws, d=(2, 1, 16, -5, 3, 4, 16)) == -1
    assert call(q, pool, bt, sl, ix, o, lse, ws, d=(2, 1, 129, 64, 3, 4, 16)) == -2    # Hq = 129
    assert call(q, pool, bt, sl, ix, o, lse, ws, d=(2, 1, 16, 64, 3, 4, 48)) == -2     # the page
    assert call(q, pool, bt, sl, ix, o, lse, ws, d=(2, 0, 16, 64, 3, 4, 16)) == -1     # T = 0
    S, _, need = _plan(DEC + "_plan", 2, 1, 16, 2048, 4, 16)[1]
    assert S == 8 and need == 2 * 16 * S * 514 * 4
    assert call(q, pool, bt, sl, ix, o, lse, ws, d=(2, 1, 16, 2048, 3, 4, 16), w=need - 1) == -1  # a workspace too small for the splits
    assert call(q, pool, bt, sl, ix, o, lse, None, d=(2, 1, 16, 2048, 3, 4, 16), w=need) == -1
    assert call(q, pool, bt, sl, ix, o, lse, ws, d=(2, 1, 129, 2048, 3, 4, 16), w=0) == -2        # the plan before the workspace


# ---------------------------------------------------------------------------------------------------- describe text

def test_describe_text_equals_its_manifest_mirror(built):
    m = built.manifest
    s = 192 ** -0.5
    for B, T, Hq, topk, mp, page in ((64, 1, 16, 200, 256, 16), (5, 2, 40, 2048, 256, 16), (8, 1, 128, 2048, 2048, 64), (3, 70, 65, 1, 4, 16)):
        rc, text = _describe(B, T, Hq, topk, mp, page, s)
        S, C, ws = sp.plan_rule(B, T, Hq, topk)
        HG = -(-Hq // 64)
        assert rc == len(text) and text == m.describe_decode_paged_mla_sparse_bf16(B, T, Hq, topk, mp, page, s)
        assert text.startswith("fa2_decode_paged_mla_sparse_bf16_mfma<Dk=576,Dv=512> ") and "v_mfma_f32_16x16x32_bf16" in text and "_f16" not in text
        s32 = float(torch.tensor(s, dtype=torch.float32))
        assert "softmax_scale=%.9g" % s32 in text and "x log2(e) = %.9g" % float(torch.tensor(s32 * ml.LOG2E, dtype=torch.float32)) in text
        assert "T=%d Hq=%d topk=%d S=%d C=%d page=%d: %d workgroups" % (T, Hq, topk, S, C, page, B * T * HG * S) in text
        assert "(sequence, query token, group of 64 heads, split of C index slots; %d head groups)" % HG in text
        assert "index -> block table entry -> latent row" in text and "72 MFMAs" in text and "64 MFMAs" in text
        assert "%d bytes static, row stride %d bytes" % (LDS, 2 * 576 + 32) in text
        assert ("fa2_decode_combine_bf16_all<D=512> merges all %d splits" % S in text and "workspace %d bytes" % ws in text) == (S > 1)
        assert (S > 1) == (topk == 2048) and text.endswith("; deterministic")
    with pytest.raises(ValueError, match="status -2"):
        m.describe_decode_paged_mla_sparse_bf16(1, 1, 129, 64, 4, 16, s)
    with pytest.raises(ValueError, match="status -1"):
        m.describe_decode_paged_mla_sparse_bf16(1, 1, 16, 0, 4, 16, s)
    with pytest.raises(ValueError, match="status -1"):
        m.describe_decode_paged_mla_sparse_bf16(1, 1, 16, 64, 4, 16, 0.0)


# ---------------------------------------------------------------------------------------------------- the Python entry

def test_python_entry_refuses_bad_tensors_before_any_device_call(built, monkeypatch):
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
    dec = built.fa2_decode_paged_mla_sparse_bf16
    good = dict(q=b(2, 3, 16, 576), pool=b(3, 16, 576), block_table=i(2, 4), seqlens=i(2), indices=i(2, 3, 64), softmax_scale=s,
                out=b(2, 3, 16, 512))
    call = lambda **kw: dec(**{**good, **kw})  # noqa: E731
    for kw in (dict(q=good["q"].half()), dict(pool=good["pool"].float()), dict(out=good["out"].half()),
               dict(seqlens=torch.zeros(2, dtype=torch.int64)), dict(indices=torch.zeros(2, 3, 64, dtype=torch.int64)),
               dict(block_table=torch.zeros(2, 4, dtype=torch.int64)), dict(lse=torch.zeros(2, 3, 16, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="values must be"):
            call(**kw)
    with pytest.raises(RuntimeError, match="q of 575 dims not supported"):
        call(q=b(2, 3, 16, 575))
    for kw in (dict(pool=b(3, 16, 512)), dict(out=b(2, 3, 16, 576)), dict(lse=torch.zeros(2, 3, 15)), dict(q=b(2, 3, 576), out=b(2, 3, 512)),
               dict(indices=i(2, 64)), dict(indices=i(2, 3, 64, 1)), dict(indices=i(2, 2, 64)), dict(indices=i(3, 3, 64)), dict(indices=i(6, 64)),
               dict(seqlens=i(3)), dict(block_table=i(3, 4)), dict(pool=b(48, 576))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            call(**kw)
    with pytest.raises(RuntimeError, match="indices must be contiguous"):
        call(indices=i(2, 3, 128)[:, :, ::2])
    with pytest.raises(RuntimeError, match="indices must be contiguous"):
        call(indices=i(3, 2, 64).transpose(0, 1))
    for bad in BAD_SCALES:
        with pytest.raises(RuntimeError, match="softmax_scale .* not supported"):
            call(softmax_scale=bad)
    with pytest.raises(TypeError):
        dec(good["q"], good["pool"], good["block_table"], good["seqlens"], good["indices"], None, good["out"])  # there is no default
    with pytest.raises(RuntimeError, match="129 query heads not supported"):
        call(q=b(2, 3, 129, 576), out=b(2, 3, 129, 512))
    with pytest.raises(RuntimeError, match="page size 48"):
        call(pool=b(3, 48, 576))
    S, _, need = built.fa2_decode_paged_mla_sparse_bf16_plan(2, 3, 16, 2048, 4, 16)
    assert S > 1
    with pytest.raises(RuntimeError, match="workspace of %d bytes, the plan needs %d" % (need - 2, need)):
        call(indices=i(2, 3, 2048), workspace=torch.zeros(need // 2 - 1, dtype=torch.int16))
    # a good call reaches the C entry, T = 9 included
    monkeypatch.setattr(host, "_ext_fn", reached)
    monkeypatch.setattr(host, "_decode_plan", lambda cname, dims: (0, (1, 64, 0)))
    with pytest.raises(Reached, match=DEC):
        call()
    with pytest.raises(Reached, match=DEC):
        call(q=b(2, 9, 16, 576), out=b(2, 9, 16, 512), indices=i(2, 9, 1), lse=torch.zeros(2, 9, 16))


# ---------------------------------------------------------------------------------------------------- registers and instructions

def _built_kernels(tmp_path):
    """{kernel name: metadata block} of the gfx950 code objects inside the built product library (llvm-objdump --offloading, llvm-readelf)."""
    from cuda_learn_notes_amd import _loader
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(objdump) and os.path.exists(readelf)
    local = str(tmp_path / "libcln_amd.so")
    shutil.copy(_loader.so_path("libcln_amd.so"), local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    out = {}
    for co in sorted(glob.glob(local + ".*gfx950")):
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
        if "mla_sparse" not in notes:
            continue
        for blk in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, "- .agpr_count" + blk).group(1))
                         for k in ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                   "group_segment_fixed_size")}
    return out


def test_kernel_resources_in_the_built_library(built, tmp_path):
    """One workgroup per CU (__launch_bounds__(256, 1)): the unified file of 512 registers, no spill, no scratch, and the LDS the describe
    text states -- read from the code objects inside the built library."""
    got = _built_kernels(tmp_path)
    stream = [(n, k) for n, k in got.items() if "fa2_decode_paged_mla_sparse_bf16_mfma" in n]
    combine = [(n, k) for n, k in got.items() if "fa2_decode_combine_bf16_all" in n]
    assert len(stream) == 1 and len(combine) == 1, sorted(got)
    for n, k in stream + combine:
        print(n, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
    k = stream[0][1]
    assert k["vgpr_count"] <= 512 and k["group_segment_fixed_size"] == LDS == 75776 and LDS <= fs.LDS_PER_CU, k
    assert "%d bytes static" % k["group_segment_fixed_size"] in _describe(5, 2, 40, 2048, 256, 16, 0.07)[1]
    assert "ILi512E" in combine[0][0] and combine[0][1]["group_segment_fixed_size"] == 0


def test_kernel_mfmas_are_the_siblings(tmp_path):
    """The loop's MFMAs per wave: 4 key blocks x 18 k-steps for S^T plus 32 dim blocks x 2 key pairs for O^T = 72 + 64 = 136, all bf16
    16x16x32, as in fa2_decode_paged_mla_bf16_mfma; the flags are read as four ds_read_b32 per step."""
    got = fs._bodies(UNIT + ".hip", tmp_path)  # asserts no spill, no scratch
    for k, _ in got:
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds", "spill", "sgpr_spill", "scratch")})
    stream = [(k, b) for k, b in got if "fa2_decode_paged_mla_sparse_bf16_mfma" in k["name"]]
    assert len(stream) == 1 and len(got) == 2, [k["name"] for k, _ in got]
    k, body = stream[0]
    assert k["lds"] == LDS and k["vgpr"] <= 512, k
    assert fs._loop_mfmas(body) == 4 * (576 // 32) + (512 // 16) * 2 == 136
    assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body and "ds_write_b8" in body
    assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", "")


# ---------------------------------------------------------------------------------------------------- a scale that is not the data's

@pytest.mark.parametrize("scale", ml.OTHER_SCALES, ids=["yarn", "quarter"])
@pytest.mark.parametrize("case", ml.SCALE_TH, ids=lambda c: "T%dxHq%d%s" % (c[0], c[1], "-split" if c[2] else ""))
def test_the_gpu_cases_at_another_scale_would_notice_the_datas_scale(case, scale):
    """tests/test_gpu_paged_mla_sparse.py runs these cases at V3's YaRN scale and at SCALE / 4 with q x Q_MULT: a kernel that ran at SCALE
    whatever it was given would be more than 20 x o_bound from the reference."""
    ref, ref0 = sp.scale_case(*case, scale)[4:]
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla sparse scale %.5f %s: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, case, diff, need))
    assert diff > need
