"""The layout plan of the large-pool tests of the latent (MLA) cache (tests/test_paged_mla_large_pool_plan.py proves it on the CPU,
tests/test_gpu_paged_mla_large_pool.py runs the MLA entries on it): tests/paged_large_pool.py generalised to a page whose element count is no
power of two. Plain Python.

Geometry: page = 16, row = 576: E = 9216 elements per page, s bytes per element (2: bf16, 1: e4m3). ONE device byte buffer of
paged_large_pool.BUF_BYTES backs the pool: the contiguous [P, 16, 576] view that starts BASE = 16 bytes in, P = pages(E, s) the most that fit.

Every kernel forms ((pg << page_shift) + row) 576 + col in 64 bits. One that formed it, or the byte offset behind it, in 32 bits would address
element (n E + r) mod M of the pool instead of element n E + r of page n, M = 2^32 elements or 2^32 / s elements. E does not divide M, so the wrap
of a page does not land on a page start: the elements of a page n with n E >= M land in the page a = ((n E) mod M) // E and, unless (n E) mod M is
a multiple of E, in the page a + 1 (a power-of-two E divides M: only a, paged_large_pool.images' n mod (M / E)); those of a page that straddles M
(n E < M < (n + 1) E) stay where they are below M and land in page 0 above it; a page below M has no image. plan() poisons every image of every
named page, its two neighbours and pages 0 .. 7, and names no page that is an image of another: a wrapped offset lands on poison (NaN, or the
e4m3 NaN byte), never on another named page.

A boundary 2^k elements (k = 31, 32; s = 1: and 33) lies inside a page, b = 2^k // E: "the page at the boundary" straddles it. The named pages
are drawn in paged_large_pool.plan's order with its replacement rule until n_live are found: page P - 1; the neighbourhood b - 2 .. b + 1 of
every boundary; the last pages P - 2, P - 3, ... A candidate that is an image of a named page, or one of whose images is named, is passed over
for the nearest free page below it (b - 2, b - 1) or, what the power-of-two geometries never need, above it (b, b + 1).

One thing a page of 9216 elements makes impossible, and the arithmetic is short. 2^31 = 233016 E + 8192 and 2^32 = 466033 E + 7168, so the byte
wrap of a bf16 pool (M = 2^31 elements) sends page 466033, the one at 2^32, to element 233016 E + 1024: into pages 233016 and 233017, the one at
2^31 and the one above it. An e4m3 pool has the same collision one boundary up (2^33 = 932067 E + 5120: the page at 2^33 wraps into the pages at
and above 2^32). The page at the highest boundary and the page at the boundary below it cannot both be named. So the plan has two orders:
top_first = False walks the boundaries lowest first, as paged_large_pool.plan does, names the whole neighbourhood of every boundary but the
highest, and above the highest names the first two free pages past its page (both wholly past the boundary); top_first = True starts at the
highest boundary, names its whole neighbourhood with the page at it, and moves the two pages at and above the boundary below it upward. Every
boundary has two named pages below it and two at or above it in either order; the GPU test runs every entry under both. A plain module: nothing
here is collected."""
import random

import paged_large_pool as lp

PAGE, ROW = 16, 576
E = PAGE * ROW
BASE, BUF_BYTES, LOW_PAGES, NEIGHBOURHOOD = lp.BASE, lp.BUF_BYTES, lp.LOW_PAGES, lp.NEIGHBOURHOOD
REACH = 8  # how far from its candidate a replacement page may lie


def pages(E, s):
    """P of the pool view: the whole pages that fit behind BASE."""
    return (BUF_BYTES - BASE) // (E * s)


def boundaries(E, s):
    """The pages in which the element offset reaches 2^31, 2^32 and, in an e4m3 pool, 2^33: they straddle the boundary unless E divides it."""
    return [(1 << k) // E for k in ((31, 32, 33) if s == 1 else (31, 32))]


def moduli(s):
    """What a 32-bit element offset and a 32-bit byte offset wrap at, in elements."""
    return (1 << 32, (1 << 32) // s)


def images(n, E, s):
    """Where a kernel whose element or byte offset wraps at 32 bits would look for the elements of page n; n itself is left out. Never fewer
    pages than the wrap reaches (the plan test compares with brute force), at most a + 1 more."""
    out = set()
    for M in moduli(s):
        a = (n * E) % M
        if n * E >= M:
            out.add(a // E)
            if a % E:
                out.add(a // E + 1)
        if a + E > M:  # the page straddles M, or its wrapped elements do: those past M land at the start of the pool
            out.add(0)
    return sorted(out - {n})


def wholly_past(n, E, k):
    """Page n lies wholly at or past element 2^k."""
    return n * E >= 1 << k


def plan(E, s, n_live, seed=0, top_first=False):
    """{"P", "named" (n_live pages, seeded shuffle), "poison" (sorted), "dead" (the poison page a table entry past the live pages points at),
    "must" (P - 1 and, per boundary, the lowest named page at or above its page and the highest named page below it)}."""
    P = pages(E, s)
    named, shadow = [], set()  # shadow: the wrap images of the named pages

    def take(n):
        if len(named) >= n_live or not LOW_PAGES <= n < P or n in named or n in shadow:
            return False
        im = images(n, E, s)
        if any(i in named for i in im):
            return False
        named.append(n)
        shadow.update(im)
        return True

    take(P - 1)
    bs = boundaries(E, s)
    for b in (bs[::-1] if top_first else bs):
        for d in NEIGHBOURHOOD:
            n, step = b + d, (-1 if d < 0 else 1)
            while len(named) < n_live and LOW_PAGES <= n < P and not take(n):
                n += step
    n = P - 2
    while len(named) < n_live and n >= LOW_PAGES:
        take(n)
        n -= 1
    assert len(named) == n_live, (E, s, n_live, len(named))
    poison = set(range(LOW_PAGES))
    for n in named:
        poison.update(images(n, E, s))
        poison.update(m for m in (n - 1, n + 1) if 0 <= m < P)
    poison -= set(named)
    must = [P - 1]
    for b in bs:
        must += [min(n for n in named if n >= b), max(n for n in named if n < b)]
    must = list(dict.fromkeys(must))
    random.Random(seed).shuffle(named)
    return {"P": P, "named": named, "poison": sorted(poison), "dead": 3, "must": must}


def last_offset(n, E, s):
    """(element offset, byte offset inside the pool view) of the last element of page n."""
    return (n + 1) * E - 1, ((n + 1) * E - 1) * s
