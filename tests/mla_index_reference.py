"""Helpers of the DSA indexer tests (tests/test_mla_index_surface.py, tests/test_gpu_mla_index.py): the fp64 reference of
cuda_learn_notes_amd.mla_index_logits_paged_bf16 with its derived bound, the exact reference of mla_index_topk, the reference of
kv_append_paged_index_bf16, and the case builders.

    logit[b, t, j] = sum_h w[b, t, h] max(0, q[b, t, h] . k[j])     for 0 <= j < vis(b, t) = clamp(len_b, 0, cap) - (T - 1 - t)

(paged_mla_sparse_reference.visible with Nmax = cap). The bound is derived, not tuned:

    |logit - ref| <= 2^-23 (128 + 64 + 2) A,     A = sum_h |w_h| sum_d |q_hd k_d|   (fp64)

bf16 x bf16 products are exact in fp32; at most 127 additions in the dot product, one multiply by w and 63 additions over the heads, each with
relative error at most 2^-23 (which also covers a matrix pipe that truncates); ReLU is 1-Lipschitz and passes the error through.

The top-k reference: a stable sort on (-logit, position) with -0 taken as +0, the first topk, then ascending positions, padded with -1; the
dense list when n <= topk.

Pools are shuffled behind their block tables in the manner of paged_mla_reference.make_pool, with NaN in EVERY pool row no sequence lists --
the rows behind a sequence's length in its last page included -- and every table entry past a sequence's pages naming a page of NaNs.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools
import random

import torch

import paged_mla_reference as ml
import paged_mla_sparse_reference as sp

BF = torch.bfloat16
D, MAX_HEADS, CHUNK, WAVE_KEYS, SCAN_BLOCK = 128, 64, 1024, 256, 4096
NAN = float("nan")
EPS_TERMS = 128 + 64 + 2
visible = sp.visible


# ---------------------------------------------------------------------------------------------------- pools

def make_pool(dense, page, lens, seed=0, spare=3):
    """(pool [P,page,d], block_table int32 [B,max_pages]) of dense rows [B,Nmax,d]: the live pages placed by a seeded permutation among `spare`
    pages that stay NaN; every row at or past len_b is NaN; every table entry past ceil(len_b / page) names a NaN page."""
    B, Nmax, d = dense.shape
    max_pages = Nmax // page
    assert max_pages * page == Nmax
    live = [(b, i) for b in range(B) for i in range(-(-min(max(lens[b], 0), Nmax) // page))]
    P = len(live) + spare
    order = list(range(P))
    random.Random(seed).shuffle(order)
    pool = torch.full((P, page, d), NAN, dtype=dense.dtype)
    bt = torch.empty(B, max_pages, dtype=torch.int32)
    nan_pages = order[len(live):]
    for b in range(B):
        for i in range(max_pages):
            bt[b, i] = nan_pages[(b + i) % spare]
    for (b, i), p in zip(live, order):
        bt[b, i] = p
        n = min(page, lens[b] - i * page)
        pool[p, :n] = dense[b, i * page:i * page + n]
    return pool, bt


def gather(pool, bt, lens):
    """Dense [B, Nmax, d] from the pool: rows at or past len_b are NaN."""
    B, max_pages = bt.shape
    page = pool.shape[1]
    out = torch.full((B, max_pages * page, pool.shape[2]), NAN, dtype=pool.dtype)
    for b in range(B):
        for i in range(-(-min(max(int(lens[b]), 0), max_pages * page) // page)):
            out[b, i * page:(i + 1) * page] = pool[int(bt[b, i])]
    return out


# ---------------------------------------------------------------------------------------------------- logits

def logits_ref(q, w, pool, bt, lens, ld, relu="inside"):
    """(ref fp64 [B,T,ld], bound fp64 [B,T,ld], vis): NaN / 0 at the positions at or past vis. relu: "inside" (the contract), "none", or
    "after" the head sum -- the two wrong readings the surface test proves distinguishable."""
    B, T, Hi, _ = q.shape
    cap = min(bt.shape[1] * pool.shape[1], ld)
    vis = visible(lens, T, cap)
    dense = gather(pool, bt, lens).double()
    ref = torch.full((B, T, ld), NAN, dtype=torch.float64)
    bound = torch.zeros(B, T, ld, dtype=torch.float64)
    qd, wd = q.double(), w.double()
    for b in range(B):
        top = max(vis[b])
        if top <= 0:
            continue
        k = dense[b, :top]
        assert bool(torch.isfinite(k).all())
        s = torch.einsum("thd,jd->thj", qd[b], k)
        a = torch.einsum("th,thj->tj", wd[b].abs(), torch.einsum("thd,jd->thj", qd[b].abs(), k.abs()))
        if relu == "inside":
            lg = torch.einsum("th,thj->tj", wd[b], s.clamp_min(0))
        elif relu == "none":
            lg = torch.einsum("th,thj->tj", wd[b], s)
        else:
            lg = torch.einsum("th,thj->tj", wd[b], s).clamp_min(0)
        for t in range(T):
            n = max(vis[b][t], 0)
            ref[b, t, :n] = lg[t, :n]
            bound[b, t, :n] = a[t, :n] * EPS_TERMS * 2.0 ** -23
    return ref, bound, vis


# ---------------------------------------------------------------------------------------------------- top-k

def topk_row(vals, topk):
    """The list of one row of n visible fp32 logits (no NaN): int32 [topk]."""
    n = vals.shape[0]
    out = torch.full((topk,), -1, dtype=torch.int32)
    if n <= topk:
        out[:n] = torch.arange(n, dtype=torch.int32)
        return out
    v = vals.double() + 0.0  # -0 + 0 = +0
    order = torch.sort(-v, stable=True).indices[:topk]
    out[:] = torch.sort(order).values.to(torch.int32)
    return out


def topk_ref(logits, lens, topk):
    """int32 [B,T,topk] of logits fp32 [B,T,ld]; cap = ld."""
    B, T, ld = logits.shape
    vis = visible(lens, T, ld)
    return torch.stack([torch.stack([topk_row(logits[b, t, :max(vis[b][t], 0)], topk) for t in range(T)]) for b in range(B)])


def topk_brute(vals, topk):
    """The definition, in plain Python: the topk first under (logit descending, position ascending), ascending, padded with -1."""
    v = [float(x) + 0.0 for x in vals]
    n = len(v)
    if n <= topk:
        return list(range(n)) + [-1] * (topk - n)
    return sorted(sorted(range(n), key=lambda j: (-v[j], j))[:topk])


# ---------------------------------------------------------------------------------------------------- append

def append_ref(pool, bt, lens_after, cu, k_new):
    """The pool after kv_append_paged_index_bf16: packed row cu[b] + i at position lens_after[b] - T_b + i, bit for bit."""
    out = pool.clone()
    page = pool.shape[1]
    Nmax = bt.shape[1] * page
    for b in range(len(lens_after)):
        Tb = cu[b + 1] - cu[b]
        for i in range(Tb):
            pos = lens_after[b] - Tb + i
            if 0 <= pos < Nmax:
                out[int(bt[b, pos // page]), pos % page] = k_new[cu[b] + i]
    return out


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test

ONE_LENS, ONE_NMAX = ml.ONE_LENS, ml.ONE_NMAX
ONE_HT = [(1, 1), (16, 3), (17, 8), (64, 33), (64, 1), (17, 33), (16, 8), (1, 3)]  # every Hi and every T of the issue, twice each
LONG_LENS, LONG_NMAX, LONG_HT, LONG_PAGE = [4000, 2048, 300, 100, 0], 4096, (64, 3), 16
TOPKS = [1, 63, 64, 65, 2048]


def _keys(B, Nmax, seed):
    return torch.randn(B, Nmax, D, generator=torch.Generator().manual_seed(seed)).to(BF)


def _queries(B, T, Hi, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, Hi, D, generator=g).to(BF)
    w = (torch.randn(B, T, Hi, generator=g) * (Hi * D) ** -0.5).float()  # both signs
    return q, w


@functools.lru_cache(maxsize=None)
def one_case(Hi, T, page):
    """(q, w, (pool, bt), lens, ld): the family's edge lengths at Nmax 320; ld = 320."""
    q, w = _queries(len(ONE_LENS), T, Hi, 100 * Hi + T + page)
    return q, w, make_pool(_keys(len(ONE_LENS), ONE_NMAX, 7), page, ONE_LENS, seed=Hi + T), ONE_LENS, ONE_NMAX


@functools.lru_cache(maxsize=None)
def long_case():
    """Nmax 4096, lengths 4000, 2048, 300, 100, 0: four key chunks of 1024, a ragged last chunk, a ragged last wave and block."""
    Hi, T = LONG_HT
    q, w = _queries(len(LONG_LENS), T, Hi, 5)
    return q, w, make_pool(_keys(len(LONG_LENS), LONG_NMAX, 9), LONG_PAGE, LONG_LENS, seed=2), LONG_LENS, LONG_NMAX


@functools.lru_cache(maxsize=None)
def reference(case, *args):
    q, w, (pool, bt), lens, ld = (one_case if case == "one" else long_case)(*args)
    return logits_ref(q, w, pool, bt, lens, ld)


@functools.lru_cache(maxsize=None)
def exact_case(Hi=64, T=3, page=16):
    """Integer q and k in [-4, 4], weights +- 2^e, e in -2 ... 2: every partial sum is a multiple of 1/4 below 2^24 / 4, so every logit is
    computed without rounding whatever the order."""
    g = torch.Generator().manual_seed(77)
    B = len(ONE_LENS)
    q = torch.randint(-4, 5, (B, T, Hi, D), generator=g).to(BF)
    k = torch.randint(-4, 5, (B, ONE_NMAX, D), generator=g).to(BF)
    w = (2.0 ** torch.randint(-2, 3, (B, T, Hi), generator=g).float()) * (torch.randint(0, 2, (B, T, Hi), generator=g).float() * 2 - 1)
    return q, w, make_pool(k, page, ONE_LENS, seed=4), ONE_LENS, ONE_NMAX


def topk_ns(topk):
    """The row lengths of the top-k cases: 0, 1, topk - 1, topk, topk + 1, the scan block +- 1, 5000."""
    return sorted({0, 1, max(topk - 1, 0), topk, topk + 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 5000})


TOPK_LD = 5008
VALUE_SETS = ["equal", "two", "low8", "high8", "special", "ties"]


@functools.lru_cache(maxsize=None)
def topk_case(topk, kind):
    """(logits fp32 [B,1,TOPK_LD], lens): one row per n of topk_ns, NaN at every j >= n."""
    ns = topk_ns(topk)
    g = torch.Generator().manual_seed(topk + 13 * VALUE_SETS.index(kind))
    B = len(ns)
    if kind == "equal":
        x = torch.full((B, TOPK_LD), 0.375)
    elif kind == "two":  # the tie class of the greater value starts topk - 10 positions in front of the scan-block edge
        x = torch.full((B, TOPK_LD), -1.5)
        x[:, max(SCAN_BLOCK - topk + 10, 0):] = 2.25
    elif kind == "low8":  # keys that differ in their lowest 8 bits only, both signs of the exponent part fixed
        x = (torch.randint(0, 256, (B, TOPK_LD), generator=g, dtype=torch.int32) | 0x3F800000).view(torch.float32)
    elif kind == "high8":  # keys that differ in their highest 8 bits only: sign and 7 exponent bits (bit 23 is 0: no inf, no NaN)
        hi = torch.randint(0, 256, (B, TOPK_LD), generator=g, dtype=torch.int64) << 24
        x = (((hi | 0x00345678) + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).view(torch.float32)
    elif kind == "special":
        pick = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-45, -1e-45, 1e-40, -3e-39, 1.0, -1.0, 3.5, -2.5, 1e38, -1e38])
        x = pick[torch.randint(0, len(pick), (B, TOPK_LD), generator=g)]
    else:  # heavy ties among 17 values
        x = torch.randint(-8, 9, (B, TOPK_LD), generator=g).float() / 4
    x = x.clone()
    assert not bool(torch.isnan(x).any())
    for b, n in enumerate(ns):
        x[b, n:] = NAN
    return x[:, None, :].contiguous(), ns
