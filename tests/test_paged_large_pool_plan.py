"""CPU: the layout plan of the large-pool tests (tests/paged_large_pool.py) does what tests/test_gpu_paged_large_pool.py relies on, for every
geometry, element size and number of live pages used there. This is the mutation argument of those tests, made without a GPU: a kernel whose
element or byte offset wraps at 32 bits reads or writes a poison page, never another named page, and the named pages do cross 2^31, 2^32 and (e4m3)
2^33 and reach the end of a pool of more than 2^32 elements. The figures are printed before they are asserted (pytest -s)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_large_pool as lp  # noqa: E402

N_LIVE = (15, 20, 256)  # the attention cases, the append cases, the several-splits cases of tests/test_gpu_paged_large_pool.py
INDEX_N_LIVE = (13, 40, 404)  # the append problem, one_case(17, 3, 16) and long_case() of tests/test_gpu_mla_index_large_pool.py
GEOMETRIES = [(Hkv, D, s) for Hkv in (2, 1) for D in lp.DS for s in (2, 1)]  # Hkv = 1: the several-splits cases


@pytest.mark.parametrize("n_live", N_LIVE)
@pytest.mark.parametrize("Hkv,D,s", GEOMETRIES)
def test_named_pages_cross_the_boundaries_and_every_wrap_lands_on_poison(Hkv, D, s, n_live):
    _check(Hkv, D, s, n_live)


@pytest.mark.parametrize("n_live", INDEX_N_LIVE)
def test_the_plan_holds_for_the_index_key_pool(n_live):
    """The DSA indexer's pool [P, 16, 128] in bf16 (tests/test_gpu_mla_index_large_pool.py): E = 2048, s = 2, the geometry of Hkv = 2, D = 64
    above, at the page counts of its cases; P = 2^21 + 16, and the view ends within 16 pages past element 2^32."""
    assert lp.page_elems(64, 2) == 16 * 128 and lp.pages(2048, 2) == 2 ** 21 + 16
    _check(2, 64, 2, n_live)


def _check(Hkv, D, s, n_live):
    E = lp.page_elems(D, Hkv)
    p = lp.plan(E, s, n_live, seed=n_live)
    P, named, poison = p["P"], p["named"], set(p["poison"])
    top = max(named)
    elem, byte = lp.last_offset(top, E, s)
    print("Hkv=%d D=%d s=%d n_live=%d: P=%d, %d named (max %d), %d poison; last element %d, last byte %d = 2^33 + %d"
          % (Hkv, D, s, n_live, P, len(named), top, len(poison), elem, byte, byte - 2 ** 33))
    assert len(named) == n_live == len(set(named))
    assert not set(named) & poison
    assert all(0 <= n < P for n in named) and all(0 <= n < P for n in poison) and p["dead"] in poison
    assert P * E * s + lp.BASE <= lp.BUF_BYTES < (P + 1) * E * s + lp.BASE
    # the end of the pool: past element 2^32 (2^33 bytes of an e4m3 pool; a 2-byte pool is past both)
    assert top == P - 1
    assert (byte if s == 1 else elem) >= 2 ** (33 if s == 1 else 32) and byte + lp.BASE < lp.BUF_BYTES
    assert elem >= 2 ** 32
    # every boundary has two named pages below it and the two at and above it
    for b in lp.boundaries(E, s):
        assert b in named and b + 1 in named, (b, sorted(named))
        below = [n for n in named if b - 8 <= n < b]
        assert len(below) >= 2, (b, sorted(named))
    # the wrap images: poison, whatever the page; and at or above a period there are two of them or one that serves both
    pe, pb = lp.periods(E, s)
    wrapped = 0
    for n in named:
        for period in (pe, pb):
            if n >= period:
                wrapped += 1
                assert n % period != n and n % period in poison, (n, period)
        assert all(i in poison for i in lp.images(n, E, s)), n
        assert all(m in poison or m in named for m in (n - 1, n + 1) if m < P), n
    assert wrapped >= 4
    assert set(range(lp.LOW_PAGES)) <= poison


def test_the_plan_is_a_function_of_its_arguments():
    E = lp.page_elems(64)
    a, b, c = lp.plan(E, 2, 20, seed=1), lp.plan(E, 2, 20, seed=1), lp.plan(E, 2, 20, seed=2)
    assert a == b and sorted(a["named"]) == sorted(c["named"]) and a["named"] != c["named"]
