"""The layout plan of the large-pool tests (tests/test_paged_large_pool_plan.py proves it on the CPU, tests/test_gpu_paged_large_pool.py runs the
paged entries on it): which pages of a pool of more than 2^32 elements a case's block table names, and which pages hold poison. Plain Python.

Geometry: Hkv = 2, page = 16, D in {64, 128}; E = Hkv page D elements per page, s bytes per element (2: fp16 / bf16, 1: e4m3). One pair of device
byte buffers of BUF_BYTES = 8 GiB + 64 KiB + 16 backs every pool: a pool is the contiguous [P, Hkv, page, D] view that starts BASE = 16 bytes into
its buffer, P = pages(E, s) the most that fit. The 2-byte views end past element 2^32 (and so past byte 2^33), the e4m3 views past byte 2^33.

Every kernel forms ((pg Hkv + kvh) page + row) D + off in 64 bits. A kernel that formed it, or the byte offset behind it, in 32 bits would address
page n mod (2^32 / E) or n mod (2^32 / (E s)) instead of page n. plan() names pages on both sides of every 2^31 / 2^32 (/ 2^33) element boundary
and at the end of the pool, and poisons both wrap images of every named page, its two neighbours and pages 0 .. 7: a wrapped offset lands on
poison (NaN, or the e4m3 NaN byte), never on another named page, and the results are no longer finite and no longer those of the small pool.

The named pages are drawn, in this order, until n_live are found: page P - 1; the neighbourhood b - 2 .. b + 1 of every boundary b = 2^31 / E,
2^32 / E (s = 1: and 2^33 / E), lowest boundary first; the last pages P - 2, P - 3, ... A candidate is passed over when it is a wrap image of a
page already named or one of its images is: b - 2 and b - 1 of the next boundary up are the images of those of the one below (2^32 / E - 1 is
2^31 / E - 1 under the byte wrap of a 2-byte pool), so those two are replaced by the nearest pages below them that are free, b - 3, b - 4, ...;
every boundary keeps two named pages below it and two at and above it. A plain module: nothing here is collected."""
import random

HKV, PAGE = 2, 16
DS = (64, 128)
BASE = 16
BUF_BYTES = (8 << 30) + (64 << 10) + 16
LOW_PAGES = 8          # pages 0 .. 7 always hold poison
NEIGHBOURHOOD = (-2, -1, 0, 1)


def page_elems(D, Hkv=HKV):
    """E; the several-splits cases have one KV head."""
    return Hkv * PAGE * D


def pages(E, s):
    """P of the pool view: the whole pages that fit behind BASE."""
    return (BUF_BYTES - BASE) // (E * s)


def boundaries(E, s):
    """The pages at which the element offset reaches 2^31, 2^32 and, in an e4m3 pool, 2^33."""
    return [(1 << k) // E for k in ((31, 32, 33) if s == 1 else (31, 32))]


def periods(E, s):
    """(pages per 2^32 elements, pages per 2^32 bytes): what a 32-bit element offset and a 32-bit byte offset wrap at."""
    return (1 << 32) // E, (1 << 32) // (E * s)


def images(n, E, s):
    """Where a kernel whose element or byte offset wraps at 32 bits would look for page n; n itself is left out (no wrap below the period)."""
    return sorted({n % p for p in periods(E, s)} - {n})


def plan(E, s, n_live, seed=0):
    """{"P", "named" (n_live pages, seeded shuffle), "poison" (sorted), "dead" (the poison page a table entry past the live pages points at)}."""
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
    for b in boundaries(E, s):
        for d in NEIGHBOURHOOD:
            n = b + d
            if d >= 0:  # at and above the boundary no page is passed over: their images are low pages (asserted by the plan test)
                take(n)
                continue
            while len(named) < n_live and n >= LOW_PAGES and not take(n):
                n -= 1
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
    random.Random(seed).shuffle(named)
    return {"P": P, "named": named, "poison": sorted(poison), "dead": 3}


def last_offset(n, E, s):
    """(element offset, byte offset inside the pool view) of the last element of page n."""
    return (n + 1) * E - 1, ((n + 1) * E - 1) * s
