"""CPU: the packed ("varlen") DSA step (include/cln_amd_ext.h: cln_mla_index_logits_paged_varlen_bf16[_fp8], cln_mla_index_topk_varlen,
cln_fa2_decode_paged_mla_sparse_varlen_bf16[_fp8] with their describe and plan entries; csrc/dsa_varlen_row.cuh and the five *_varlen_*
compile units) -- header, exports and package, every status that returns before a device call in its documented order, the
sparse plan against the fixed-T plan, the describe texts against their manifest mirrors, the model of the clamped binary search against the
brute-force definition, the per-sequence references against the fixed-T ones on a uniform batch, and the five kernels' resources and loop
MFMA counts against their fixed-T siblings'. No GPU needed: every refusal returns before a launch, and hipcc cross-compiles."""
import ctypes
import glob
import itertools
import os
import random
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
import dsa_varlen_reference as dv  # noqa: E402
import mla_index_reference as ix  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of the built library and of a code object)

LOGITS, LOGITS8, TOPK = "cln_mla_index_logits_paged_varlen_bf16", "cln_mla_index_logits_paged_varlen_bf16_fp8", "cln_mla_index_topk_varlen"
SPARSE, SPARSE8 = "cln_fa2_decode_paged_mla_sparse_varlen_bf16", "cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8"
ENTRIES = (LOGITS, LOGITS8, TOPK, SPARSE, SPARSE8)
NAMES = ENTRIES + tuple(n + "_describe" for n in ENTRIES) + (SPARSE + "_plan", SPARSE8 + "_plan")
UNITS = ("mla_index_logits_paged_varlen_bf16", "mla_index_logits_paged_varlen_bf16_fp8", "mla_index_topk_varlen",
         "flash_attn_decode_paged_mla_sparse_varlen_bf16", "flash_attn_decode_paged_mla_sparse_varlen_bf16_fp8")
I, LL, VP, F = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_float
LOGITS_ARGS = [VP] * 7 + [I] * 3 + [LL] + [I] * 3 + [VP]
TOPK_ARGS = [VP] * 4 + [I] * 2 + [LL, I, VP]
SPARSE_ARGS = [VP] * 9 + [LL] + [I] * 7 + [F, VP]
SPARSE8_ARGS = [VP] * 10 + [LL] + [I] * 7 + [F, VP]
BF = torch.bfloat16
LDS_SPARSE = 64 * (2 * 576 + 32)
_fn, _plan = fs._fn, fs._plan


# ---------------------------------------------------------------------------------------------------- the search

def _offsets():
    """Well-formed offsets: every B of the issue, T_b = 0 runs at the front, in the middle and at the back, cu_q[0] > 0, cu_q[B] < total_q."""
    rnd = random.Random(11)
    yield dv.RAGGED_CU, dv.RAGGED_TOTAL
    yield dv.SINGLE_CU, dv.SINGLE_TOTAL
    yield dv.EMPTY_CU, dv.EMPTY_TOTAL
    for B in (1, 2, 3, 7, 8, 9):
        for front, back in ((0, 0), (3, 0), (0, 2), (1, 4)):
            for _ in range(6):
                Ts = [rnd.choice((0, 0, 1, 2, 5)) for _ in range(B)]
                for zeros in ("front", "middle", "back"):
                    T2 = list(Ts)
                    lo = {"front": 0, "middle": B // 3, "back": B - max(B // 3, 1)}[zeros]
                    for b in range(lo, min(lo + max(B // 3, 1), B)):
                        T2[b] = 0
                    cu = [front + sum(T2[:b]) for b in range(B + 1)]
                    yield cu, max(cu[-1] + back, 1)


def test_search_model_is_the_brute_force_definition():
    count = empties = 0
    for cu, total_q in _offsets():
        c, Ts = dv.clamped(cu, total_q)
        owners = []
        for r in range(total_q):
            got = dv.find_row(cu, total_q, r)
            assert got == dv.row_brute(cu, total_q, r), (cu, total_q, r)
            owners.append(got)
            count += 1
        # every token of every sequence is exactly one packed row, in order
        assert [o[:2] for o in owners if o is not None] == [(b, t) for b in range(len(Ts)) for t in range(Ts[b])], cu
        empties += sum(o is None for o in owners)
    assert count > 2000 and empties > 300
    rows = dv.rows(dv.RAGGED_CU, dv.RAGGED_TOTAL)
    assert rows[:2] == [None, None] and rows[-3:] == [None] * 3 and rows[2] == (1, 0, 1) and rows[3:6] == [(2, t, 3) for t in range(3)]
    assert rows[6] == (4, 0, 70) and rows[75] == (4, 69, 70) and rows[76:78] == [(5, 0, 2), (5, 1, 2)]
    assert dv.no_sequence_rows(tuple(dv.RAGGED_CU), dv.RAGGED_TOTAL) == (0, 1, 78, 79, 80)
    assert dv.rows(dv.EMPTY_CU, dv.EMPTY_TOTAL) == [None] * 3 and dv.rows(dv.SINGLE_CU, dv.SINGLE_TOTAL) == [None, (0, 0, 3), (0, 1, 3), (0, 2, 3), None, None]


def test_search_model_on_malformed_offsets_names_only_its_own_row():
    """Decreasing, negative and too large offsets: monotone after the clamp the search is still the definition; decreasing ones are outside
    the contract, and whatever the search returns is a token (b, t) with 0 <= t < T_b whose packed row c[b] + t is r itself."""
    rnd = random.Random(3)
    cases = [(cu, dv.RAGGED_TOTAL) for cu in dv.MALFORMED.values()]
    for _ in range(300):
        B = rnd.choice((1, 2, 3, 7, 8, 9))
        cases.append(([rnd.randint(-20, 60) for _ in range(B + 1)], rnd.randint(1, 40)))
    seen = 0
    for cu, total_q in cases:
        c, Ts = dv.clamped(cu, total_q)
        for r in range(total_q):
            got = dv.find_row(cu, total_q, r)
            if c == sorted(c):
                assert got == dv.row_brute(cu, total_q, r), (cu, total_q, r)
            if got is not None:
                b, t, T = got
                assert 0 <= b < len(Ts) and T == Ts[b] and 0 <= t < T and c[b] + t == r, (cu, total_q, r, got)
                seen += 1
    assert seen > 500
    assert sorted(dv.clamped(dv.MALFORMED["negative"], 81)[0]) == dv.clamped(dv.MALFORMED["negative"], 81)[0]
    assert dv.clamped(dv.MALFORMED["too_large"], 81)[0][-2:] == [81, 81]


def test_per_sequence_references_are_the_fixed_t_ones_on_a_uniform_batch():
    g = torch.Generator().manual_seed(2)
    B, T, Hi, ld, lens, topk = 3, 4, 5, 48, [40, 2, 17], 8
    q = torch.randn(B, T, Hi, ix.D, generator=g).to(BF)
    w = torch.randn(B, T, Hi, generator=g).float()
    pool, bt = ix.make_pool(torch.randn(B, 48, ix.D, generator=g).to(BF), 16, lens, seed=1)
    cu = dv.uniform_cu(B, T)
    ref, bound, _ = ix.logits_ref(q, w, pool, bt, lens, ld)
    pr, pb = dv.logits_ref(q.reshape(B * T, Hi, ix.D), w.reshape(B * T, Hi), pool, bt, lens, cu, ld)
    assert torch.equal(torch.isnan(pr), torch.isnan(ref.reshape(B * T, ld))) and torch.equal(pr.nan_to_num(), ref.reshape(B * T, ld).nan_to_num())
    assert torch.equal(pb, bound.reshape(B * T, ld))
    lg = ref.nan_to_num().float()
    assert torch.equal(dv.topk_ref(lg.reshape(B * T, ld), lens, cu, topk), ix.topk_ref(lg, lens, topk).reshape(B * T, topk))
    assert dv.vis_rows(lens, cu, B * T, 48) == [v for row in sp.visible(lens, T, 48) for v in row]
    # the ragged batch is what its comment says
    vis = dv.vis_rows(dv.RAGGED_LENS, dv.RAGGED_CU, dv.RAGGED_TOTAL, dv.NMAX)
    assert vis[2] == 1023 and vis[3:6] == [0, 1, 2] and vis[6:76] == list(range(31, 101)) and vis[76:78] == [1024, 1025]
    assert all(v is None for r, v in enumerate(vis) if r in (0, 1, 78, 79, 80))


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_twelve_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    lg = "const void*, const float*, const void*, const int*, const int*, const int*, float*, int, int, int, long long, int, int, int, void*"
    ld = "int, int, int, long long, int, int, char*, int"
    pl = "int, int, int, int, int, int*, int*, long long*"
    sd = "int, int, int, int, int, int, float, char*, int"
    tail = "void*, float*, void*, long long, int, int, int, int, int, int, int, float, void*"
    protos = {LOGITS: lg, LOGITS8: lg, TOPK: "const float*, const int*, const int*, int*, int, int, long long, int, void*",
              SPARSE: "const void*, const void*, const int*, const int*, const int*, const int*, " + tail,
              SPARSE8: "const void*, const void*, const int*, const int*, const int*, const float*, const int*, " + tail,
              LOGITS + "_describe": ld, LOGITS8 + "_describe": ld, TOPK + "_describe": "int, int, long long, int, char*, int",
              SPARSE + "_describe": sd, SPARSE8 + "_describe": sd, SPARSE + "_plan": pl, SPARSE8 + "_plan": pl}
    assert set(protos) == set(NAMES)
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, protos[n], n) for i, n in enumerate(NAMES))
                   + "int main(void) { return %s ? 0 : 1; }\n" % " && ".join("f%d" % i for i in range(len(NAMES))))
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_package_host_and_build_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ENTRIES + (SPARSE + "_plan", SPARSE8 + "_plan"):
        assert hasattr(built, n[4:]) and hasattr(host, n[4:]), n
    for n in ENTRIES:
        assert hasattr(built.manifest, "describe_" + n[4:].replace("fa2_", "")), n
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    for u in UNITS:
        assert '"%s.hip"' % u in build and all(os.path.exists(os.path.join(fs.CSRC, u + e)) for e in (".hip", ".cuh")), u
        assert '#include "dsa_varlen_row.cuh"' in open(os.path.join(fs.CSRC, u + ".cuh")).read(), u  # one search, included by all five
    assert sum("while (lo < hi)" in open(os.path.join(fs.CSRC, u + ".cuh")).read() for u in UNITS) == 0


# ---------------------------------------------------------------------------------------------------- the plan

def test_sparse_plan_is_the_fixed_t_plan_of_the_same_rows(built):
    shapes = list(itertools.product((1, 3, 64), (1, 4, 70, 2048), (1, 17, 65, 128), (64, 65, 2048), ((128, 16), (512, 64))))
    shapes += [(2, 3, 129, 64, (128, 16)), (2, 3, 128, 64, (128, 48)), (2, 3, 0, 64, (128, 16)), (2, 3, 64, 0, (128, 16)), (1 << 16, 1 << 15, 1, 64, (128, 16))]
    several = 0
    for B, T, Hq, topk, (mp, page) in shapes:
        want = _plan("cln_fa2_decode_paged_mla_sparse_bf16_plan", B, T, Hq, topk, mp, page)
        if B * T < 1 << 31:
            for name in (SPARSE, SPARSE8):
                assert _plan(name + "_plan", B * T, Hq, topk, mp, page) == want, (name, B, T, Hq, topk, mp, page)
            if want[0] == 0:
                assert want[1] == sp.plan_rule(B, T, Hq, topk) == built.fa2_decode_paged_mla_sparse_varlen_bf16_plan(B * T, Hq, topk, mp, page)
                several += want[1][0] > 1
    assert several > 20
    assert _plan(SPARSE + "_plan", 0, 64, 64, 128, 16) == (-1, (-7, -7, -7)) and _plan(SPARSE8 + "_plan", 5, 129, 64, 128, 16) == (-2, (-7, -7, -7))
    assert built.fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan(81, 128, 2048, 128, 16) == built.fa2_decode_paged_mla_sparse_varlen_bf16_plan(81, 128, 2048, 128, 16)
    with pytest.raises(RuntimeError, match="129 query heads not supported"):
        built.fa2_decode_paged_mla_sparse_varlen_bf16_plan(5, 129, 64, 128, 16)
    with pytest.raises(RuntimeError, match="page size 48"):
        built.fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan(5, 128, 64, 128, 48)


# ---------------------------------------------------------------------------------------------------- statuses

def _ptrs(n):
    buf = (ctypes.c_char * (256 * (n + 1)))()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    return buf, [base + 256 * i for i in range(n)]


@pytest.mark.parametrize("name", [LOGITS, LOGITS8])
def test_logits_statuses_in_their_order(built, name):
    """Pointers (q_idx, idx_pool 16 bytes; weights, block_table, seqlens, cu_q, logits 4), output equal to an input, P, non-positive
    dimensions, then the -2s. Nothing is launched before a refusal."""
    fn = _fn(name, LOGITS_ARGS)
    keep, ptrs = _ptrs(7)
    dims = (2, 6, 64, 320, 5, 20, 16)  # B, total_q, Hi, ld, P, max_pages, page
    bad_hi = (2, 6, 65, 320, 5, 20, 16)
    call = lambda *a, d=dims: fn(*a, *d, None)  # noqa: E731
    for i in range(7):  # a missing pointer, cu_q (5) among them, ahead of an unsupported shape
        args = list(ptrs)
        args[i] = None
        assert call(*args) == -1 and call(*args, d=bad_hi) == -1, i
    for i, off in ((0, 8), (1, 2), (2, 8), (3, 2), (4, 2), (5, 2), (6, 2)):  # misaligned, one by one
        args = list(ptrs)
        args[i] += off
        assert call(*args) == -1 and call(*args, d=bad_hi) == -1, i
    q, w, pool, bt, sl, cu, lg = ptrs
    assert call(q, w + 4, pool, bt + 4, sl + 4, cu + 4, lg + 4, d=(2, 6, 64, 320, 0, 20, 16)) == -1  # 4-byte aligned passes: P is next
    assert call(q, w + 4, pool, bt + 4, sl + 4, cu + 4, lg + 4, d=bad_hi) == -2
    for i in range(6):  # the output equal to an input
        args = list(ptrs)
        args[6] = args[i]
        assert call(*args, d=bad_hi) == -1, i
    assert call(*ptrs, d=(2, 6, 65, 320, 0, 20, 16)) == -1  # P ahead of the shape
    for d in ((0, 6, 64, 320, 5, 20, 16), (2, 0, 64, 320, 5, 20, 16), (2, -3, 65, 320, 5, 20, 48), (2, 6, 0, 320, 5, 20, 16), (2, 6, 64, 0, 5, 20, 16),
              (2, 6, 64, 320, 5, 0, 16), (2, 6, 64, 320, 5, 20, 0), (-1, 6, 65, 320, 5, 20, 16)):
        assert call(*ptrs, d=d) == -1, d
    for d in (bad_hi, (2, 6, 64, 320, 5, 20, 48), (2, 6, 64, 320, 5, 1 << 23, 256), ((1 << 31) - 1, (1 << 31) - 1, 64, 1 << 20, 5, 1 << 22, 256)):
        assert call(*ptrs, d=d) == -2, d  # Hi, the page, max_pages page, the grid
    dsc = _fn(name + "_describe", [I, I, I, LL, I, I, ctypes.c_char_p, I])
    buf = ctypes.create_string_buffer(4096)
    assert dsc(2, 6, 64, 320, 20, 16, None, 4096) == -1 and dsc(2, 6, 64, 320, 20, 16, buf, 0) == -1 and dsc(0, 6, 64, 320, 20, 16, buf, 4096) == -1
    assert dsc(2, 6, 65, 320, 20, 16, buf, 4096) == -2 and dsc(2, 0, 65, 320, 20, 16, buf, 4096) == -1 and dsc(2, 6, 64, 1 << 40, 20, 16, buf, 4096) > 0


def test_topk_statuses_in_their_order(built):
    fn = _fn(TOPK, TOPK_ARGS)
    keep, ptrs = _ptrs(4)
    lg, sl, cu, ix_ = ptrs
    call = lambda *a, d=(2, 6, 320, 64): fn(*a, *d, None)  # noqa: E731  B, total_q, ld, topk
    for i in range(4):
        args = list(ptrs)
        args[i] = None
        assert call(*args) == -1 and call(*args, d=(2, 6, 1 << 31, 64)) == -1, i
        args = list(ptrs)
        args[i] += 2
        assert call(*args) == -1 and call(*args, d=(2, 6, 1 << 31, 64)) == -1, i
    assert call(lg, sl, cu, lg) == -1 and call(lg, sl, cu, sl) == -1 and call(lg, sl, cu, cu) == -1  # indices aliasing an input
    assert call(lg + 4, sl + 4, cu + 4, ix_ + 4, d=(2, 6, 320, 0)) == -1 and call(lg + 4, sl + 4, cu + 4, ix_ + 4, d=(2, 6, 1 << 31, 64)) == -2
    for d in ((0, 6, 320, 64), (2, 0, 320, 64), (2, 6, 0, 64), (2, 6, 320, 0), (2, -1, 1 << 31, 64), (0, 6, 1 << 31, 64)):
        assert call(*ptrs, d=d) == -1, d
    for d in ((2, 6, 1 << 31, 64), (2, 1 << 30, 320, (1 << 31) - 1), (2, 1 << 22, 320, 64)):
        assert call(*ptrs, d=d) == -2, d  # ld, topk total_q, the grid (total_q 1024 = 2^32)
    dsc = _fn(TOPK + "_describe", [I, I, LL, I, ctypes.c_char_p, I])
    buf = ctypes.create_string_buffer(4096)
    assert dsc(2, 6, 320, 64, None, 4096) == -1 and dsc(0, 6, 320, 64, buf, 4096) == -1 and dsc(2, 6, 1 << 31, 64, buf, 4096) == -2
    assert dsc(2, (1 << 22) - 1, (1 << 31) - 1, 64, buf, 4096) > 0


@pytest.mark.parametrize("name", [SPARSE, SPARSE8])
def test_sparse_statuses_in_their_order(built, name):
    """The scale, the pointers (q, pool, o, lse, workspace 16 bytes; block_table, seqlens, cu_q, [kv_scale,] indices 4), aliasing, P, the
    shape and the plan (total_q <= 0 before Hq > 128), the workspace."""
    fp8 = name == SPARSE8
    fn = _fn(name, SPARSE8_ARGS if fp8 else SPARSE_ARGS)
    n_in = 7 if fp8 else 6
    keep, ptrs = _ptrs(n_in + 3)
    dims = (2, 6, 128, 2048, 5, 128, 16)  # B, total_q, Hq, topk, P, max_pages, page: the plan splits
    need = _plan(name + "_plan", 6, 128, 2048, 128, 16)[1][2]
    assert need > 0
    bad_hq = (2, 6, 129, 2048, 5, 128, 16)
    call = lambda *a, ws=need, d=dims, s=0.1: fn(*a, ws, *d, s, None)  # noqa: E731
    for s in (0.0, -1.0, float("nan"), float("inf")):  # the scale first, ahead of a missing pointer
        assert call(*([None] * (n_in + 3)), s=s) == -1 and call(*ptrs, s=s, d=bad_hq) == -1
    for i in range(n_in + 1):  # the inputs and o; lse may be null, the workspace is needed as the plan splits
        args = list(ptrs)
        args[i] = None
        assert call(*args) == -1 and call(*args, d=bad_hq) == -1, i
    args = list(ptrs)
    args[n_in + 1] = None
    assert call(*args, d=bad_hq) == -2  # lse is optional: the next refusal is the plan's
    args[n_in + 1], args[n_in + 2] = ptrs[n_in + 1], None
    assert call(*args) == -1  # no workspace where the plan splits
    for i in range(n_in + 3):  # misaligned, one by one: 16 bytes for q, pool, o, lse, workspace, 4 for the rest
        args = list(ptrs)
        args[i] += 2 if 2 <= i < n_in else 8
        assert call(*args, d=bad_hq) == -1, i
    args = [p + (4 if 2 <= i < n_in else 0) for i, p in enumerate(ptrs)]
    assert call(*args, d=bad_hq) == -2  # 4-byte aligned int inputs pass, cu_q among them
    for i in range(n_in):  # an output equal to an input
        args = list(ptrs)
        args[n_in] = args[i]
        assert call(*args, d=bad_hq) == -1, i
    assert call(*ptrs, d=(2, 6, 129, 2048, 0, 128, 16)) == -1  # P ahead of the plan
    for d in ((0, 6, 129, 2048, 5, 128, 16), (2, 0, 129, 2048, 5, 128, 16), (2, -6, 129, 2048, 5, 128, 48), (2, 6, 0, 2048, 5, 128, 16),
              (2, 6, 128, 0, 5, 128, 16), (2, 6, 128, 2048, 5, 0, 16), (2, 6, 128, 2048, 5, 128, 0)):
        assert call(*ptrs, d=d) == -1, d  # total_q <= 0 is refused before Hq > 128
    for d in (bad_hq, (2, 6, 128, 2048, 5, 128, 48), (2, 6, 128, 2048, 5, 1 << 23, 256)):
        assert call(*ptrs, d=d) == -2, d
    assert call(*ptrs, ws=need - 1) == -1 and call(*ptrs, ws=need - 1, d=bad_hq) == -2  # the workspace last
    dsc = _fn(name + "_describe", [I] * 6 + [F, ctypes.c_char_p, I])
    buf = ctypes.create_string_buffer(8192)
    assert dsc(2, 6, 128, 64, 128, 16, 0.1, None, 8192) == -1 and dsc(2, 6, 129, 64, 128, 16, 0.0, buf, 8192) == -1
    assert dsc(0, 6, 128, 64, 128, 16, 0.1, buf, 8192) == -1 and dsc(2, 6, 129, 64, 128, 16, 0.1, buf, 8192) == -2 and dsc(2, 6, 128, 64, 128, 16, 0.1, buf, 8192) > 0


# ---------------------------------------------------------------------------------------------------- describe texts

def test_describe_texts_equal_their_manifest_mirrors_and_state_the_packed_job_mapping(built):
    m = built.manifest
    search = "found by binary search over the device-side offsets"
    buf = ctypes.create_string_buffer(8192)
    for name, mirror in ((LOGITS, m.describe_mla_index_logits_paged_varlen_bf16), (LOGITS8, m.describe_mla_index_logits_paged_varlen_bf16_fp8)):
        dl = _fn(name + "_describe", [I, I, I, LL, I, I, ctypes.c_char_p, I])
        for B, tq, Hi, ld, mp, page in ((64, 2111, 64, 32768, 512, 64), (7, 81, 17, 2048, 128, 16), (1, 1, 1, 5000, 64, 64), (9, 16, 33, 100, 20, 16)):
            rc = dl(B, tq, Hi, ld, mp, page, buf, 8192)
            text = buf.value.decode()
            cap = min(mp * page, ld)
            chunks = -(-cap // ix.CHUNK)
            assert rc == len(text) and text == mirror(B, tq, Hi, ld, mp, page)
            assert text.startswith("%s_mfma<NHB=%d> B=%d total_q=%d Hi=%d ld=%d cap=%d page=%d: " % (name[4:], -(-Hi // 16), B, tq, Hi, ld, cap, page))
            assert "%d workgroups of 4 waves, one per (packed row, chunk of 1024 keys; %d chunks a row" % (tq * chunks, chunks) in text
            assert search in text and "%d MFMAs per block" % (4 * -(-Hi // 16)) in text and "a row of no sequence writes nothing" in text
            assert "no LDS" in text and text.endswith("; deterministic")
    dt = _fn(TOPK + "_describe", [I, I, LL, I, ctypes.c_char_p, I])
    for B, tq, ld, topk in ((64, 2111, 32768, 2048), (7, 81, 300, 1)):
        rc = dt(B, tq, ld, topk, buf, 8192)
        text = buf.value.decode()
        assert rc == len(text) and text == m.describe_mla_index_topk_varlen(B, tq, ld, topk)
        assert text.startswith("mla_index_topk_varlen_rows B=%d total_q=%d ld=%d topk=%d: " % (B, tq, ld, topk))
        assert "%d workgroups of 1024 threads, one per packed row" % tq in text and search in text and "1288 bytes of LDS" in text
        assert text.endswith("; deterministic")
    for name, mirror in ((SPARSE, m.describe_decode_paged_mla_sparse_varlen_bf16), (SPARSE8, m.describe_decode_paged_mla_sparse_varlen_bf16_fp8)):
        ds = _fn(name + "_describe", [I] * 6 + [F, ctypes.c_char_p, I])
        for B, tq, Hq, topk, mp, page in ((64, 2111, 128, 2048, 512, 64), (7, 81, 128, 2048, 128, 16), (7, 81, 17, 64, 128, 16)):
            rc = ds(B, tq, Hq, topk, mp, page, 0.1, buf, 8192)
            text = buf.value.decode()
            S, C, ws = _plan(name + "_plan", tq, Hq, topk, mp, page)[1]
            assert rc == len(text) and text == mirror(B, tq, Hq, topk, mp, page, 0.1)
            assert text.startswith(name[4:] + "_mfma<Dk=576,Dv=512> softmax_scale=") and "B=%d total_q=%d Hq=%d topk=%d S=%d C=%d page=%d: " % (B, tq, Hq, topk, S, C, page) in text
            assert "%d workgroups of 4 waves, one per (packed row, group of 64 heads" % (tq * -(-Hq // 64) * S) in text and search in text
            assert "%d bytes static" % LDS_SPARSE in text and "O = 0, LSE = -inf" in text and text.endswith("; deterministic")
            assert ("workspace %d bytes" % ws in text) == (S > 1)
    with pytest.raises(ValueError, match="status -2"):
        m.describe_mla_index_logits_paged_varlen_bf16(1, 1, 65, 320, 20, 16)
    with pytest.raises(ValueError, match="status -1"):
        m.describe_mla_index_topk_varlen(0, 1, 320, 64)
    with pytest.raises(ValueError):
        m.describe_decode_paged_mla_sparse_varlen_bf16(1, 1, 129, 64, 20, 16, 0.1)


# ---------------------------------------------------------------------------------------------------- the Python entries

def test_python_entries_refuse_bad_tensors_before_any_device_call(built, monkeypatch):
    """No GPU: the device check is replaced, and a call that gets as far as the C entry shows it by raising Reached."""
    from cuda_learn_notes_amd import host

    class Reached(Exception):
        pass

    def reached(name, argtypes):
        raise Reached(name)

    with pytest.raises(RuntimeError, match="expected a GPU"):
        built.mla_index_topk_varlen(torch.zeros(6, 320), torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 64,
                                    torch.zeros(6, 64, dtype=torch.int32))
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)
    b = lambda *sh: torch.zeros(*sh, dtype=BF)  # noqa: E731
    f = lambda *sh: torch.zeros(*sh, dtype=torch.float32)  # noqa: E731
    i = lambda *sh: torch.zeros(*sh, dtype=torch.int32)  # noqa: E731
    good = dict(q_idx=b(6, 17, 128), weights=f(6, 17), idx_pool=b(5, 16, 128), block_table=i(2, 20), seqlens=i(2), cu_q=i(3), logits=f(6, 320))
    lg = lambda **kw: built.mla_index_logits_paged_varlen_bf16(**{**good, **kw})  # noqa: E731
    lg8 = lambda **kw: built.mla_index_logits_paged_varlen_bf16_fp8(**{**good, "idx_pool": torch.zeros(5, 16, 132, dtype=torch.uint8), **kw})  # noqa: E731
    for call in (lg, lg8):
        for kw in (dict(q_idx=good["q_idx"].half()), dict(weights=good["weights"].double()), dict(idx_pool=f(5, 16, 128)),
                   dict(cu_q=torch.zeros(3, dtype=torch.int64)), dict(logits=good["logits"].half())):
            with pytest.raises(RuntimeError, match="values must be"):
                call(**kw)
        for kw in (dict(weights=f(6, 16)), dict(seqlens=i(3)), dict(cu_q=i(2)), dict(cu_q=i(4)), dict(logits=f(5, 320)), dict(logits=f(2, 3, 320)),
                   dict(q_idx=b(2, 3, 17, 128))):
            with pytest.raises(RuntimeError, match="size mismatch"):
                call(**kw)
        with pytest.raises(RuntimeError, match="65 index heads not supported"):
            call(q_idx=b(6, 65, 128), weights=f(6, 65))
    with pytest.raises(RuntimeError, match="page size 48"):
        lg(idx_pool=b(5, 48, 128))
    tk = lambda **kw: built.mla_index_topk_varlen(**{**dict(logits=f(6, 320), seqlens=i(2), cu_q=i(3), topk=64, indices=i(6, 64)), **kw})  # noqa: E731
    for kw in (dict(logits=f(6, 320).half()), dict(cu_q=torch.zeros(3, dtype=torch.int64)), dict(indices=torch.zeros(6, 64, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="values must be"):
            tk(**kw)
    for kw in (dict(indices=i(6, 63)), dict(indices=i(5, 64)), dict(indices=i(2, 3, 64)), dict(cu_q=i(2)), dict(logits=f(2, 3, 320)), dict(topk=65)):
        with pytest.raises(RuntimeError, match="size mismatch"):
            tk(**kw)
    sgood = dict(q=b(6, 5, 576), pool=b(5, 16, 576), block_table=i(2, 20), seqlens=i(2), cu_q=i(3), indices=i(6, 64), softmax_scale=0.1, out=b(6, 5, 512))
    sd = lambda **kw: built.fa2_decode_paged_mla_sparse_varlen_bf16(**{**sgood, **kw})  # noqa: E731
    sd8 = lambda **kw: built.fa2_decode_paged_mla_sparse_varlen_bf16_fp8(**{**sgood, "pool": torch.zeros(5, 16, 576).to(torch.float8_e4m3fn),  # noqa: E731
                                                                            "kv_scale": f(1), **kw})
    for call in (sd, sd8):
        for kw in (dict(q=sgood["q"].half()), dict(cu_q=torch.zeros(3, dtype=torch.int64)), dict(indices=torch.zeros(6, 64, dtype=torch.int64))):
            with pytest.raises(RuntimeError, match="values must be"):
                call(**kw)
        for kw in (dict(out=b(6, 5, 576)), dict(out=b(5, 5, 512)), dict(cu_q=i(2)), dict(seqlens=i(3)), dict(indices=i(5, 64)), dict(indices=i(2, 3, 64)),
                   dict(q=b(2, 3, 5, 576)), dict(lse=f(6, 4))):
            with pytest.raises(RuntimeError, match="size mismatch"):
                call(**kw)
        with pytest.raises(RuntimeError, match="q of 512 dims not supported"):
            call(q=b(6, 5, 512))
    monkeypatch.setattr(host, "_ext_fn", reached)  # a good call reaches the C entry
    for name, call in ((LOGITS, lg), (LOGITS8, lg8), (TOPK, tk), (SPARSE, sd), (SPARSE8, sd8)):
        with pytest.raises(Reached, match=name + "$"):
            call()


# ---------------------------------------------------------------------------------------------------- registers, LDS and MFMAs

def _built_kernels(tmp_path):
    """{kernel name: metadata} of every kernel of the DSA step in the gfx950 code objects inside the built product library."""
    from cuda_learn_notes_amd import _loader
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(objdump) and os.path.exists(readelf)
    local = str(tmp_path / "libcln_amd.so")
    shutil.copy(_loader.so_path("libcln_amd.so"), local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    out = {}
    for co in sorted(glob.glob(local + ".*gfx950")):
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
        if "mla_index" not in notes and "mla_sparse" not in notes:
            continue
        for blk in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, "- .agpr_count" + blk).group(1))
                         for k in ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                   "group_segment_fixed_size")}
    return out


def test_kernel_resources_in_the_built_library_are_the_siblings(built, tmp_path):
    """No spill, no scratch; the LDS bytes of each fixed-T sibling (0 / 0 / 1288 / 75776 / the FP8 sibling's) and the vector registers within
    the sibling's launch bounds: 256 for the logits kernels (two workgroups a CU), 128 for the top-k (1024 threads), 512 for the sparse ones."""
    got = _built_kernels(tmp_path)
    pairs = (("mla_index_logits_paged_varlen_bf16_mfma", "mla_index_logits_paged_bf16_mfma", 4, 256),
             ("mla_index_logits_paged_varlen_bf16_fp8_mfma", "mla_index_logits_paged_bf16_fp8_mfma", 4, 256),
             ("mla_index_topk_varlen_rows", "mla_index_topk_rows", 1, 128),
             ("fa2_decode_paged_mla_sparse_varlen_bf16_mfma", "fa2_decode_paged_mla_sparse_bf16_mfma", 1, 512),
             ("fa2_decode_paged_mla_sparse_varlen_bf16_fp8_mfma", "fa2_decode_paged_mla_sparse_bf16_fp8_mfma", 1, 512))
    for new, old, count, regs in pairs:
        mine = sorted((n, k) for n, k in got.items() if new in n)
        sib = sorted((n, k) for n, k in got.items() if old in n)
        assert len(mine) == count == len(sib), (new, sorted(got))
        for (n, k), (sn, sk) in zip(mine, sib):
            print(n, k, "| sibling", sk)
            assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
            assert k["group_segment_fixed_size"] == sk["group_segment_fixed_size"], (n, k, sk)
            assert k["vgpr_count"] <= regs, (n, k)
    lds = {new: [k["group_segment_fixed_size"] for n, k in got.items() if new in n][0] for new, _, _, _ in pairs}
    assert list(lds.values()) == [0, 0, 1288, LDS_SPARSE, LDS_SPARSE]


@pytest.mark.parametrize("unit", UNITS)
def test_kernel_loop_mfmas_are_the_siblings(tmp_path, unit):
    """The key loop's MFMAs per wave: 4 NHB for the logits kernels, 136 for the sparse ones, none for the top-k -- each sibling's count,
    compiled here from the sibling's own compile unit; the search adds no MFMA and no LDS instruction."""
    got = fs._bodies(unit + ".hip", tmp_path)  # asserts no spill, no scratch
    sib = fs._bodies(unit.replace("_varlen", "") + ".hip", tmp_path)
    main = [(k, b) for k, b in got if "_varlen_" in k["name"]]
    smain = [(k, b) for k, b in sib if "combine" not in k["name"]]
    assert len(main) == len(smain) == (4 if "logits" in unit else 1) and len(got) == len(sib), [k["name"] for k, _ in got]
    for (k, body), (sk, sbody) in zip(main, smain):
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds")}, "| sibling", {x: sk.get(x) for x in ("vgpr", "agpr", "sgpr", "lds")})
        assert k["lds"] == sk["lds"]
        assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", "")
        if "topk" in unit:
            assert "v_mfma" not in body and k["lds"] == 1288
            continue
        want = 4 * int(re.search(r"mfmaILi(\d)E", k["name"]).group(1)) if "logits" in unit else 136
        assert fs._loop_mfmas(body) == fs._loop_mfmas(sbody) == want, k["name"]
        assert ("ds_" in body) == ("ds_" in sbody)
