"""CPU: the layout plan of the large-pool tests of the latent cache (tests/paged_mla_large_pool.py) does what
tests/test_gpu_paged_mla_large_pool.py relies on, for both element sizes, both orders and every number of live pages from 13 to the largest used
there. This is the mutation argument of those tests, made without a GPU: a kernel whose element or byte offset wraps at 32 bits reads or writes a
poison page, never another named page, and the named pages lie on both sides of 2^31, 2^32 and (e4m3) 2^33 elements and reach the end of a pool of
more than 2^32 elements. For the power-of-two geometries of tests/test_paged_large_pool_plan.py the generalised image rule and plan are the old
ones. The figures are printed before they are asserted (pytest -s)."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_large_pool as lp  # noqa: E402
import paged_mla_large_pool as mlp  # noqa: E402
import test_paged_large_pool_plan as old  # noqa: E402

E = mlp.E
N_LIVE_MAX = 404  # the sparse several-splits case: lengths 4000, 2048, 300, 100, 0 at page 16
N_LIVE_USED = (24, 26, 40, 106, 404)  # append, gather, one split, several splits (and the fp8 gather, the chains), sparse several splits


@functools.lru_cache(maxsize=None)
def wrapped_pages(n, s):
    """Brute force: the pages the elements of page n land in when the element offset is taken mod M, for both moduli; n itself left out."""
    out = set()
    for M in mlp.moduli(s):
        for r in range(0, E, 64):  # every 64th element and the last: a page is 9216 = 144 x 64 elements, the boundaries are multiples of 64
            out.add(((n * E + r) % M) // E)
        out.add(((n * E + E - 1) % M) // E)
    return frozenset(out - {n})


def test_the_geometry():
    assert E == 9216 and E & (E - 1) != 0
    assert 2 ** 31 == 233016 * E + 8192 and 2 ** 32 == 466033 * E + 7168 and 2 ** 33 == 932067 * E + 5120
    assert mlp.boundaries(E, 2) == [233016, 466033] and mlp.boundaries(E, 1) == [233016, 466033, 932067]
    assert mlp.pages(E, 2) == 466037 and mlp.pages(E, 1) == 932074
    # the collision the two orders exist for: the page at the highest boundary wraps into the page at the boundary below it and the one above
    assert mlp.images(466033, E, 2) == [0, 233016, 233017] and mlp.images(932067, E, 1) == [0, 466033, 466034]


@pytest.mark.parametrize("top_first", [False, True], ids=["low-first", "top-first"])
@pytest.mark.parametrize("s", [2, 1], ids=["bf16", "e4m3"])
def test_named_pages_cross_the_boundaries_and_every_wrap_lands_on_poison(s, top_first):
    P = mlp.pages(E, s)
    bs = mlp.boundaries(E, s)
    top_k = 33 if s == 1 else 32
    assert P * E * s + mlp.BASE <= mlp.BUF_BYTES < (P + 1) * E * s + mlp.BASE
    for n_live in range(13, N_LIVE_MAX + 1):
        p = mlp.plan(E, s, n_live, seed=n_live, top_first=top_first)
        named, poison = p["named"], set(p["poison"])
        top = max(named)
        elem, byte = mlp.last_offset(top, E, s)
        past = sorted(n for n in named if mlp.wholly_past(n, E, top_k))
        if n_live in N_LIVE_USED or n_live == 13:
            print("s=%d %s n_live=%d: P=%d, %d named (max %d), %d poison, %s wholly past 2^%d; must %s; last element %d, last byte %d = 2^33 + %d"
                  % (s, "top first" if top_first else "low first", n_live, P, len(named), top, len(poison), past, top_k, p["must"], elem, byte,
                     byte - 2 ** 33))
        assert p["P"] == P and len(named) == n_live == len(set(named))
        assert not set(named) & poison
        assert all(mlp.LOW_PAGES <= n < P for n in named) and all(0 <= n < P for n in poison) and p["dead"] in poison
        # the end of the pool: past element 2^32 (e4m3: 2^33), and at least two named pages lie wholly past the top boundary
        assert top == P - 1 and elem >= 2 ** top_k and byte >= 2 ** 33 and byte + mlp.BASE < mlp.BUF_BYTES
        assert len(past) >= 2 and P - 1 in past
        # every boundary: two named pages below it and two at or above its page, all nearby; the page at it unless the collision forbids it
        for k, b in zip((31, 32, 33), bs):
            below = [n for n in named if b - mlp.REACH <= n < b]
            above = [n for n in named if b <= n <= b + mlp.REACH]
            assert len(below) >= 2 and len(above) >= 2, (k, b, sorted(named))
            assert all((n + 1) * E <= 1 << k for n in below) and sum(mlp.wholly_past(n, E, k) for n in above) >= 1
            collides = b == (bs[-1] if not top_first else bs[-2])
            assert (b in named) != collides, (k, b, top_first)
        assert p["must"][0] == P - 1 and set(p["must"]) <= set(named) and len(p["must"]) == 1 + 2 * len(bs)
        for i, b in enumerate(bs):
            at, under = p["must"][1 + 2 * i], p["must"][2 + 2 * i]
            assert b <= at <= b + mlp.REACH and b - mlp.REACH <= under < b
        # the wrap images: poison, whatever the page; the rule of the module against brute force
        wrapped = 0
        for n in named:
            im = set(mlp.images(n, E, s))
            assert wrapped_pages(n, s) <= im and len(im - wrapped_pages(n, s)) <= 1, (n, sorted(im))
            for M in mlp.moduli(s):
                if n * E >= M:  # the rule as the issue states it: ((n E) mod M) // E and that plus one
                    wrapped += 1
                    a = ((n * E) % M) // E
                    assert {a, a + 1} <= poison, (n, M)
            assert im <= poison and not im & set(named), n
            assert all(m in poison or m in named for m in (n - 1, n + 1) if 0 <= m < P), n
        assert wrapped >= 4
        assert set(range(mlp.LOW_PAGES)) <= poison


@pytest.mark.parametrize("s", [2, 1], ids=["bf16", "e4m3"])
def test_the_two_orders_name_the_page_at_every_boundary_between_them(s):
    for n_live in N_LIVE_USED:
        a, b = (set(mlp.plan(E, s, n_live, top_first=t)["named"]) for t in (False, True))
        assert set(mlp.boundaries(E, s)) <= a | b


@pytest.mark.parametrize("Hkv,D,s", old.GEOMETRIES)
def test_power_of_two_geometries_keep_the_old_images_and_the_old_plan(Hkv, D, s):
    E2 = lp.page_elems(D, Hkv)
    assert mlp.pages(E2, s) == lp.pages(E2, s) and mlp.boundaries(E2, s) == lp.boundaries(E2, s)
    P = lp.pages(E2, s)
    probe = sorted({n + d for n in [0, 9, P - 1] + lp.boundaries(E2, s) + list(lp.periods(E2, s)) for d in range(-3, 4) if 0 <= n + d < P})
    for n in probe:
        assert mlp.images(n, E2, s) == lp.images(n, E2, s), n
    for n_live in old.N_LIVE:
        a, b = mlp.plan(E2, s, n_live, seed=n_live), lp.plan(E2, s, n_live, seed=n_live)
        for n in a["named"]:
            assert mlp.images(n, E2, s) == lp.images(n, E2, s), n
        assert all(a[k] == b[k] for k in ("P", "named", "poison", "dead"))


def test_the_plan_is_a_function_of_its_arguments():
    a, b, c = mlp.plan(E, 2, 40, seed=1), mlp.plan(E, 2, 40, seed=1), mlp.plan(E, 2, 40, seed=2)
    assert a == b and sorted(a["named"]) == sorted(c["named"]) and a["named"] != c["named"]
