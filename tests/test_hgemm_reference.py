"""tests/hgemm_reference.py proven on the CPU before it judges a kernel: the case table reaches every HGEMM kernel family csrc/hgemm.hip can name
(manifest.describe is host code: no GPU), no case is listed under a family it does not run, the integer inputs stay exact in fp32, enough answers
are rounded ones, the K >= 4096 cases overflow to +-inf, the poison plan leaves most of C alone, and half_rne (with its inf extension) is
torch's own rounding."""
import os
import re

import pytest
import torch

import hgemm_reference as hr
import ix_reference as ix

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-learn-notes_amd", "csrc")


@pytest.fixture(scope="module")
def tb(built):
    return hr.table(built.manifest)


def all_cases(tb):
    return [c for cs in tb["cases"].values() for c in cs]


def sampled(case):
    """(a, b) of the exact case; for the large shapes the first and last 16 rows of A only (the row classes repeat every 8 rows)."""
    a, b = hr.exact_inputs(case.M, case.N, case.K)
    if case.big:
        a = torch.cat([a[:16], a[-16:]])
    return a, b


def test_every_family_the_library_can_name_is_reached(built, tb, capsys):
    """The families of describe_best / describe_ring / describe_w4, each reached through a run-time dispatched name; split-K on every tile of
    splitk_plan in both forms (256 x 256 in the reduce form only: the planner never picks its fix-up form in the search domain); both tail forms."""
    m = built.manifest
    reached = {}
    for c in all_cases(tb):
        fam = hr.expected_family(c, m)
        if fam is not None:
            reached.setdefault(fam, []).append(c.cid)
    want = set(hr.SINGLE_PASS_FAMILIES) | set(hr.TAIL_FAMILIES) | {"splitk<%s>,reduce" % t for t in hr.SPLITK_TILES}
    want |= {"splitk<%s>,fixup" % t for t in hr.SPLITK_TILES if t != "256x256"}
    with capsys.disabled():
        for fam in sorted(reached):
            print("%-36s %3d cases, e.g. %s" % (fam, len(reached[fam]), reached[fam][0]))
    assert set(reached) == want, (sorted(want - set(reached)), sorted(set(reached) - want))
    assert "splitk<256x256>,fixup" not in hr._search(m)
    # the family strings exist in the source the table was written from
    src = open(os.path.join(CSRC, "hgemm.hip")).read()
    for text in ("mfma_ring<%dx%dx%d", "hgemm_w4<%dx%dx64", "hgemm_w4s<256x256,ring of %d", "hgemm_pp<192x256x64", "hgemm_pp<256x256x64", "hgemm_pp32<256x256",
                 "split-K x %d", "tail split", "in-kernel fix-up", "hgemm_splitk_reduce"):
        assert text in src, text
    assert re.search(r"shapes\[\] = \{\{256, 256, [\d.]+\}, \{192, 256, [\d.]+\}, \{192, 192, [\d.]+\}, \{128, 256, [\d.]+\}, \{160, 160, [\d.]+\}\}", src)


def test_no_case_is_listed_under_a_family_it_does_not_run(built, tb):
    m = built.manifest
    for c in all_cases(tb):
        assert c.M % c.bm == 0 and c.N % c.bn == 0 or c.family in ("valu", "naive_mfma", "vendor"), c
        e = c.entry
        if e[0] == "g6":
            fam = hr.expected_family(c, m)
            if c.family == "splitk":
                assert fam.startswith("splitk<%dx%d>" % (c.bm, c.bn)), (c, fam)
            elif c.family == "tail":
                assert fam.startswith("tail_split"), (c, fam)
            elif c.family == "w4s":
                assert fam == "hgemm_w4s<256x256,ring of %d" % e[2], (c, fam)
            elif c.family == "w4":
                assert fam == "hgemm_w4<%dx%d" % (c.bm, c.bn), (c, fam)
            else:
                assert c.family == "dispatched" and "<%dx%d" % (c.bm, c.bn) in fam or fam == "hgemm_pp32", (c, fam)
            assert c.scheduled == (not fam.startswith("mfma_ring")), c
        elif e[0] == "variant":
            kind, tile, bk, st = e[1:]
            if kind == 0:
                assert hr.ring_fits(tile, bk, st) and hr.RING_TILES[tile][:2] == (c.bm, c.bn) and c.K % bk == 0 and c.bk == bk, c
            elif kind == 15:
                assert hr.W4_KIND15[tile] == (c.bm, c.bn) and hr.w4_k_ok(c.K), c
            elif kind == 16:
                assert hr.w4s_k_ok(c.K, st), c
            else:
                assert (kind, st) in hr.PP_VARIANTS and c.K % 64 == 0 and (c.bm, c.bn) == (256, 256), c
        elif c.family == "1stage" and e[1] in hr.ONE_STAGE_SWITCH:
            assert hr.one_stage_form(c.M, c.N, c.K) == (c.bm, c.bn, c.bk), c
    forms = {hr.one_stage_form(c.M, c.N, c.K)[0] for c in tb["cases"]["1stage"] if c.entry[1] in hr.ONE_STAGE_SWITCH and c.K == 64 and c.M >= 1920}
    assert forms == {64, 128}  # both sides of the switch of launch_1stage_128_or_64
    # the LDS skips are those of tests/test_gpu_hgemm.py test_every_ring_instantiation (the same formula on the same budget)
    for tile, layout, bk, st in tb["lds_skips"]:
        assert st * {0: 256, 1: 512, 2: 384, 3: 384, 6: 192, 7: 128, 8: 128}[tile] * bk * 2 > 160 * 1024
    assert len(tb["lds_skips"]) == 14


def test_the_mirrors_are_the_sources(built):
    """Constants and rules of hgemm_reference.py that mirror a launcher, line by line."""
    def has(fn, text):
        assert text in open(os.path.join(CSRC, fn)).read(), (fn, text)
    has("hgemm_w4.cuh", "inline bool w4_k_ok(int K) { return K % 64 == 0 && K >= ((K / 64) & 1 ? 448 : 384); }")
    has("hgemm_w4s.cuh", "inline bool w4s_k_ok(int K, int S) { return K % 64 == 0 && K / 32 >= 2 * S; }")
    has("hgemm.hip", "if ((long long)(M / 128) * (N / 128) < 256 && M % 64 == 0 && N % 64 == 0 && K % 64 == 0)")
    has("hgemm_valu.cuh", "if (M % 128 || N % 128 || K % BK) return CLN_ERR_UNSUPPORTED;")
    has("hgemm_mfma.cuh", "if (K % 4) return CLN_ERR_UNSUPPORTED;")
    has("hgemm_ring_impl.inc", "constexpr int kLdsLimit = 160 * 1024;")
    for tile, (BM, BN, WM, WN) in hr.RING_TILES.items():
        has("hgemm_ring_impl.inc", "return exact<%d, %d, %d, %d>(bk, S, a, b, c, M, N, K, swz, stride, st);" % (BM, BN, WM, WN))
    for tile, (BM, BN) in hr.W4_KIND15.items():
        has("probe/hgemm_probe.hip", "if (tile == %d) { W4_SHAPE(%d, %d) }" % (tile, BM, BN))
    src = open(os.path.join(CSRC, "hgemm.hip")).read()
    for name, (BK, TM) in hr.VALU_TILE_RUNGS.items():
        assert re.search(r"CLN_G3\(%s,\s*\(launch_valu_tile<%d, %d, " % (name, BK, TM), src), name
    insts = set(re.findall(r"launch_valu_tile<(\d+, \d+, \w+, \w+)>", src))
    mine = set(re.search(r"CLN_G3\(%s,\s*\(launch_valu_tile<(\d+, \d+, \w+, \w+)>" % n, src).group(1) for n in hr.VALU_TILE_RUNGS)
    assert insts == mine  # one name per distinct instantiation, none left out


def test_exact_inputs_stay_exact_and_round(built, tb):
    seen = {}
    for c in all_cases(tb):
        key = (c.M, c.N, c.K)
        if key in seen:
            continue
        a, b = sampled(c)
        r = hr.magnitude(c.K)
        assert c.K * r * r < (1 << 24), c  # every output, every order
        assert int(a.abs().max()) <= r and int(b.abs().max()) <= r
        assert hr.abs_sum_bound(a, b) < (1 << 24), c
        prod = hr.int_product(a, b)
        share = hr.rounded_share(prod)
        seen[key] = share
        assert hr.rounding_possible(c.K), c  # (the table has no K at which a rounded answer is out of reach)
        assert share >= 0.1, (c, share)
        want = hr.half_rne(prod)
        if c.K >= 4096:
            assert bool(torch.isinf(want).any()) and bool((want == float("inf")).any()) and bool((want == -float("inf")).any()), c
            assert float(torch.isinf(want).double().mean()) < 0.5, c
        assert not torch.isnan(want).any()
    assert len(seen) > 100


def test_int_product_is_the_int64_product():
    for (M, N, K) in ((64, 64, 64), (100, 100, 64), (9, 20, 20), (128, 256, 4096), (192, 192, 4736)):
        a, b = hr.exact_inputs(M, N, K)
        exact = a.to(torch.int64) @ b.to(torch.int64)
        assert torch.equal(hr.int_product(a, b), exact)
        assert hr.abs_sum_bound(a, b) == ix.abs_sum_bound(a, b) == int((a.abs().double() @ b.abs().double()).max())
        assert torch.equal(hr.expected_exact(a, b).view(torch.int16), exact.double().to(torch.float16).view(torch.int16))


def test_half_rne_is_torchs_rounding_with_inf_from_65520_on():
    v = torch.arange(-70000, 70001, dtype=torch.int64)  # spans every tie of [2048, 65536) and both infinities
    assert torch.equal(hr.half_rne(v).view(torch.int16), v.double().to(torch.float16).view(torch.int16))
    got = hr.half_rne(torch.tensor([65519, 65520, 65536, -65519, -65520, 1 << 24, 2049, 2051])).double().tolist()
    assert got == [65504.0, float("inf"), float("inf"), -65504.0, -float("inf"), float("inf"), 2048.0, 2052.0]


def test_poison_plan_sits_on_the_edges_and_leaves_most_of_c_alone(built, tb):
    for c in all_cases(tb):
        if c.family == "vendor":
            continue
        rows, cols = hr.poison_plan(c)
        ms, ns, ks = [m for m, _ in rows], [n for n, _ in cols], hr.poison_ks(c)
        assert {0, c.M - 1} <= set(ms) and {0, c.N - 1} <= set(ns), c
        assert set(ms) >= {i for i in (15, 16, c.wtm - 1, c.wtm, c.bm - 1, c.bm) if i < c.M}, c
        assert set(ns) >= {i for i in (15, 16, c.wtn - 1, c.wtn, c.bn - 1, c.bn) if i < c.N}, c
        assert {0, c.K - 1, min(c.bk, c.K) - 1} <= set(ks) and all(0 <= k < c.K for k in ks), c
        if c.K > c.bk:
            assert (c.K - 1) // c.bk * c.bk in ks, c  # the first element of the last K tile
        used = {k for _, k in rows} | {k for _, k in cols}
        assert used == set(ks) or len(rows) + len(cols) < len(ks), c
        free = 1.0 - float(hr.poison_mask(c).double().mean())
        assert free >= 0.5, (c, free)


def test_special_values_are_exactly_representable(built, tb):
    """The builder asserts it; here it runs for every distinct small shape of the table (and one large one), and the answers hold every class."""
    seen = set()
    for c in all_cases(tb):
        key = (c.M, c.N, c.K)
        if key in seen or c.K < 8 or (c.big and len([k for k in seen if k[0] * k[1] > (1 << 20)]) >= 1):
            continue
        seen.add(key)
        a, b, want = hr.special_inputs(c)
        assert a.dtype == b.dtype == torch.float16
        sub = (a != 0) & (a.abs() < 2.0 ** -14)
        assert sub.any() and ((b != 0) & (b.abs() < 2.0 ** -14)).any()  # subnormal inputs on both sides
        if c.M >= hr.SPECIAL_ROW_KINDS:
            w = want[:8]
            assert ((w != 0) & (w.abs() < 2.0 ** -14)).any() and (w == 65504.0).any() and (w == float("inf")).any() and (w == -float("inf")).any()
            assert torch.isnan(w).any() == (c.N >= 4)
    assert len(seen) > 50


def test_refused_shapes_are_refused_by_the_rule_the_table_names(built, tb):
    for r in tb["refused"]:
        e = r.entry
        if e[0] == "g3" and e[1] in hr.VALU_TILE_RUNGS:
            assert r.M % 128 or r.N % 128 or r.K % hr.VALU_TILE_RUNGS[e[1]][0], r
        elif e[0] == "g3" and e[1] in hr.ONE_STAGE_SWITCH:
            assert hr.one_stage_form(r.M, r.N, r.K) is None, r
        elif e[0] == "g3" and e[1] == hr.ONE_STAGE_64x128:
            assert r.M % 64 or r.N % 128 or r.K % 32, r
        elif e[0] == "g3":
            assert r.K % 4, r
        elif e[1] == 15:
            assert not hr.w4_k_ok(r.K), r
        else:
            assert e[1] == 16 and not hr.w4s_k_ok(r.K, e[4]), r
