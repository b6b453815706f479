"""CPU: the tables of tests/paged_edge_cases.py are what tests/test_gpu_paged_edge_counts.py needs them to be. (a) `visible` agrees with the
references the randn tests use (multi_decode_reference.visible, prefill_reference.visible, and the lower edge max(0, n - W) /
paged_window_reference.lo_min of paged_window_reference) on every row of every case; (b) the tables reach every residue mod 16 of both edges
and of the count, every structural size r with -1, 0 and +1, every split case splits, and every (entry, D) has every table that applies to
it; (c) every defect of the model changes the expected count of some row in every table it applies to; (d) the criterion of the randn tests
does not see a count that is off by one at the largest n of the tables, and the counting bound does -- both numbers are in the message."""
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_decode_reference as mr  # noqa: E402
import paged_all_entries as ae  # noqa: E402
import paged_edge_cases as ec  # noqa: E402
import paged_window_reference as wr  # noqa: E402
import prefill_reference as pf  # noqa: E402

NAMES = [e.name for e in ec.ENTRIES]


def all_cases(name, D):
    return [c for tb in ec.tables_of(ae.BY_NAME[name]) for c in ec.TABLES[tb](name, D)]


def test_the_sixteen_entries_and_their_tables(built):
    """(b), the last clause: every (entry, D) appears in each table that applies to it."""
    assert len(NAMES) == 16 == len(set(NAMES))
    for suffix in ("bf16", "window_bf16", "window_sink_bf16", "window_sink_bf16_fp8", "window_sink_anyg_bf16", "window_sink_anyg_bf16_fp8",
                   "window_sink_softcap_anyg_bf16", "window_sink_softcap_anyg_bf16_fp8"):
        assert "fa2_prefill_paged_varlen_" + suffix in NAMES and "fa2_decode_paged_multi_" + suffix in NAMES
    for name in NAMES:
        e = ae.BY_NAME[name]
        for D in ec.DS:
            for tb in ec.tables_of(e):
                cases = ec.TABLES[tb](name, D)
                assert cases and all(c.table == tb for c in cases), (name, D, tb)
                assert {c.page for c in cases} >= ({16, 256} if tb == "split" else set(ec.PAGES)), (name, D, tb)
                assert {c.W for c in cases} >= (set(ec.windows(e, 16)) if tb != "split" else {None}), (name, D, tb)
                if e.window and tb == "split":
                    assert any(c.W is not None for c in cases), (name, D)
            assert ec.onehot_cases(name, D)


@pytest.mark.parametrize("name", NAMES)
def test_visible_is_the_references_mask(built, name):
    """(a)"""
    rows = 0
    for D in ec.DS:
        for c in all_cases(name, D):
            W = wr.INT_MAX if c.W is None else c.W
            vis = ec.counts(c)
            if c.T is not None:
                want = mr.visible(list(c.lens), c.T, c.Nmax)
                assert want == pf.visible(list(c.lens), c.T, c.Nmax).flatten().tolist()
            else:
                want = [int(x) for b, T in enumerate(c.Ts) for x in pf.visible([c.lens[b]], T, c.Nmax)[0].tolist()]
            assert len(want) == len(vis)
            for (b, t, T), v, n in zip(ec.rows_of(c), vis, want):
                lo = max(0, n - W)  # paged_window_reference._sequence
                assert (v.hi + 1 if v.n else 0) == n, (name, c, b, t)
                assert v.n == n - lo and (v.lo == lo or not v.n), (name, c, b, t)
                if t == 0 and v.n:
                    assert v.lo == wr.lo_min(min(max(c.lens[b], 0), c.Nmax), T, W), (name, c, b)
            rows += len(vis)
    assert rows > 1000


@pytest.mark.parametrize("D", ec.DS)
@pytest.mark.parametrize("name", NAMES)
def test_the_tables_reach_every_residue_every_edge_and_every_split(built, name, D):
    """(b)"""
    e = ae.BY_NAME[name]
    his, los, ns = set(), set(), set()
    for tb in ec.tables_of(e):
        cases = ec.TABLES[tb](name, D)
        at_len, at_first = set(), set()
        for c in cases:
            if tb == "split":
                assert c.S > 1 and ec.plan_of(e, len(c.lens), c.T, c.G * c.Hkv, c.Hkv, c.Nmax // c.page, c.page, D, c.W)[:2] == (c.S, c.C), c
                rel = set()
                for n in c.lens:
                    L = min(max(n, 0), c.Nmax)
                    rel.add(L - ec.base_of(L, c.T, c.W, c.page))
                if c.W is None:
                    assert {k * c.C + d for k in (1, 2, c.S - 1, c.S) for d in (-1, 0, 1)} - {c.S * c.C + 1} <= rel, c  # S C + 1 is past Nmax
                    assert c.S * c.C == c.Nmax and any(n > c.Nmax for n in c.lens)            # ... and is there as a clamped length
                    assert any(0 < n <= (c.S - 2) * c.C for n in c.lens)                       # the last splits stay empty
                else:
                    assert {c.C + d for d in (-1, 0, 1)} <= rel, c
                    if ec.unit(c.page) == c.C:  # the lower edge can reach a chunk boundary only where a chunk is one unit
                        lo_rel = {(ec.visible(n, c.T, 0, c.W, c.Nmax).lo - ec.base_of(n, c.T, c.W, c.page)) % c.C for n in c.lens
                                  if ec.base_of(n, c.T, c.W, c.page) > 0}
                        assert {c.C - 1, 0, 1} <= lo_rel, (c, lo_rel)
            elif tb == "one":
                assert c.S == 1, c
                assert {0, 1, c.T - 1, c.T, c.Nmax} <= set(c.lens) and min(c.lens) < 0 and max(c.lens) > c.Nmax, c
            else:
                assert 0 in c.Ts and any(0 < n < T for n, T in zip(c.lens, c.Ts)) and any(n > c.Nmax for n in c.lens), c
                rows = [T * c.G for T in c.Ts]
                assert any(0 < r < ec.ROW_TILE for r in rows) and any(r > ec.ROW_TILE for r in rows), c
                assert c.G in (3, 7, 12) or not e.anyg
            for (b, t, T), v in zip(ec.rows_of(c), ec.counts(c)):
                L = min(max(c.lens[b], 0), c.Nmax)
                if t == 0:
                    at_first.add(L - T)
                at_len.add(L)
                if v.n:
                    his.add((v.hi + 1) % 16), los.add(v.lo % 16), ns.add(v.n % 16)
        rs = ec.PREFILL_RS if tb == "prefill" else ec.RS
        if tb != "split":
            for page in ec.PAGES:
                for r in rs(page):
                    for d in (-1, 0, 1):
                        # the last row's upper edge is len - 1: "len at the edge" of the decode tables, "p at the edge" of the prefill table
                        assert (r + d + (tb == "prefill")) in at_len and (r + d) in at_first, (name, D, tb, r, d)
        if tb == "prefill":
            assert {c.G for c in cases} == set(ec.prefill_groups(e)) or not e.window
    want = set(range(16))
    assert his == want and ns == want and (los == want or not e.window), (name, D, his, los, ns)


@pytest.mark.parametrize("name", NAMES)
def test_every_defect_changes_a_count_in_every_table_it_applies_to(built, name):
    """(c): and the changed count is seen by the counting bound, which separates n from every other integer."""
    e = ae.BY_NAME[name]
    for D in ec.DS:
        for tb in ec.tables_of(e):
            cases = ec.TABLES[tb](name, D)
            for defect in ec.DEFECTS:
                mine = [c for c in cases if ec.applies(defect, c)]
                if not mine:
                    assert defect in ec.WINDOW_DEFECTS + ec.CHUNK_DEFECTS, (name, tb, defect)
                    continue
                moved = 0
                for c in mine:
                    for good, bad in zip(ec.counts(c), ec.counts(c, defect)):
                        if good.n != bad.n:
                            moved += 1
                            if good.n and bad.n > 0:
                                assert abs(math.log(bad.n) - math.log(good.n)) > 2 * ec.count_bound(good.n), (name, c, defect, good, bad)
                assert moved, (name, D, tb, defect)


def test_the_randn_criterion_does_not_see_an_off_by_one_and_the_counting_bound_does(built):
    """(d)"""
    top = max(v.n for name in NAMES for D in ec.DS for c in all_cases(name, D) for v in ec.counts(c))
    moves = (math.log(top + 1) - math.log(top), math.log(top) - math.log(top - 1))
    old, new = ec.lse_tol_at(top), ec.count_bound(top)
    msg = ("largest n of the tables %d: one key more or less moves ln n by %.3e / %.3e; decode_reference.lse_tol there is %.3e (it passes), the "
           "counting bound 1 / (4 (n + 1)) is %.3e (it fails)" % (top, moves[0], moves[1], old, new))
    print(msg)
    assert top >= 1024, msg
    assert max(moves) < old, msg
    assert min(moves) > 2 * new, msg  # a kernel that is n +- 1 is more than its own bound away from ln n as well
    for n in (1, 2, 7, 100, top):
        assert ec.count_bound(n) < (math.log(n + 1) - math.log(n)) / 2


def test_the_one_hot_margin_holds_for_every_identity_case(built):
    for name in NAMES:
        e = ae.BY_NAME[name]
        for D in ec.DS:
            x = ec.onehot_scale(e, D)[0] if e.softcap else 1.0 / math.sqrt(D)
            for c in ec.onehot_cases(name, D):
                score, margin = ec.onehot_score(c.Nmax, D, x)
                assert margin >= ec.ONEHOT_MARGIN and D // ec.code_bits(c.Nmax) >= 1, (name, D, c.Nmax, margin)
                k = ec.codes(c.Nmax, D).double()
                s = (16.0 * k[-1:] @ k.T)[0] * x
                assert float(s[-1]) == score and float(s[:-1].max()) <= score - margin * (1 - 1e-12)
