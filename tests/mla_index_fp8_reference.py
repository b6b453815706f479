"""Helpers of the tests of the DSA indexer's FP8 cache (tests/test_mla_index_fp8_surface.py, tests/test_gpu_mla_index_fp8.py,
tests/test_gpu_mla_index_fp8_large_pool.py): the pool layout, the CPU reference of
cuda_learn_notes_amd.kv_append_paged_index_bf16_fp8 in the kernel's fp32 operations, the fp64 reference of mla_index_logits_paged_bf16_fp8
with its derived bound and with the wrong readings the surface test proves distinguishable, and the case builders.

The pool is torch.uint8 [P, page, 132]; inside a page of 132 page bytes the codes [page,128] e4m3fn come first (slot r at byte 128 r), the
scales [page] fp32 behind them (slot r at byte 128 page + 4 r). A stored token means k_d = e4m3(code_d) scale.

The append, per live token, all in fp32: a = max(amax |k|, 1e-4); scale = a / 448; with scale_pow2 the smallest power of two >= scale, on
the integer view of the bits (mantissa zero: unchanged; else exponent + 1, mantissa 0); codes = fp8_kv_reference.quantize(k, scale).

    logit[b, t, j] = s_j sum_h w[b, t, h] max(0, q[b, t, h] . c_j)     for 0 <= j < vis(b, t)

in fp64 on the dequantised pool, with the bound, derived, not tuned:

    |logit - ref| <= 2^-23 (128 + 64 + 3) A,     A = s_j sum_h |w_h| sum_d |q_hd c_jd|

-- mla_index_reference's derivation (bf16 x bf16 products exact in fp32, and every e4m3 code is a bf16 value; at most 127 additions in the
dot product, one multiply by w and 63 additions over the heads, each at most 2^-23 relative) plus one rounding for the scale.

Pools are built as mla_index_reference.make_pool builds them: every unlisted code byte is 0x7F (e4m3fn NaN), every unlisted scale NaN, and
table entries past a sequence's pages name such a page. A plain module: nothing here is collected. Cases are made on the CPU, once per
process, and never modified."""
import functools
import random

import torch

import fp8_kv_reference as fk
import mla_index_reference as ix

BF, F8 = torch.bfloat16, fk.F8
D, ROW = ix.D, 132
NAN, NAN_BYTE = ix.NAN, fk.NAN_BYTE
EPS_TERMS = 128 + 64 + 3
FLOOR = 1e-4
visible = ix.visible
MODES = ("right", "no_scale", "next_slot", "other_page", "relu_after", "relu_none")


# ---------------------------------------------------------------------------------------------------- the pool

def views(pool):
    """(codes float8_e4m3fn [P,page,128], scales float32 [P,page]): views of the storage of pool uint8 [P,page,132], written here from the
    layout and not through the package."""
    P, page, row = pool.shape
    assert pool.dtype == torch.uint8 and row == ROW and pool.is_contiguous()
    pages = pool.view(P, page * ROW)
    return pages[:, :page * D].view(F8).view(P, page, D), pages[:, page * D:].view(torch.float32)


def empty_pool(P, page):
    """A pool of P pages in which no token is stored: every code byte 0x7F, every scale NaN."""
    pool = torch.empty(P, page, ROW, dtype=torch.uint8)
    codes, scales = views(pool)
    codes.view(torch.uint8).fill_(NAN_BYTE)
    scales.fill_(NAN)
    return pool


def token_scales(k, pow2):
    """fp32 [n] of bf16 rows k [n,128], in the kernel's fp32 operations."""
    a = k.float().abs().amax(dim=-1).clamp_min(torch.tensor(FLOOR, dtype=torch.float32))
    s = a / torch.tensor(448.0, dtype=torch.float32)
    if pow2:
        b = s.view(torch.int32)
        s = torch.where((b & 0x007FFFFF) != 0, (b & 0x7F800000) + 0x00800000, b).view(torch.float32)
    return s


def quantise_rows(k, pow2):
    """(codes e4m3fn [n,128], scales fp32 [n]) of bf16 rows k [n,128]."""
    s = token_scales(k, pow2)
    return fk.quantize(k, s[:, None]), s


def append_ref(pool, bt, lens_after, cu, k_new, pow2):
    """The pool bytes after kv_append_paged_index_bf16_fp8: which row goes where is mla_index_reference.append_ref's; every byte that is not
    a live token's 128 codes or 4 scale bytes keeps its value."""
    out = pool.clone()
    codes, scales = views(out)
    P, page = pool.shape[:2]
    Nmax = bt.shape[1] * page
    c, Ts = ix.append_clamped(cu, k_new.shape[0])
    kc, ks = quantise_rows(k_new, pow2)
    for b in range(len(lens_after)):
        for i in range(Ts[b]):
            pos = lens_after[b] - Ts[b] + i
            if 0 <= pos < Nmax and 0 <= int(bt[b, pos // page]) < P:
                pg, r = int(bt[b, pos // page]), pos % page
                codes.view(torch.uint8)[pg, r] = kc[c[b] + i].view(torch.uint8)
                scales[pg, r] = ks[c[b] + i]
    return out


def make_pool(codes, scales, page, lens, seed=0, spare=3):
    """(pool uint8 [P,page,132], block_table int32 [B,max_pages]) of dense codes e4m3fn [B,Nmax,128] and scales fp32 [B,Nmax], placed as
    mla_index_reference.make_pool places its rows: a seeded permutation among `spare` pages that stay empty (0x7F codes, NaN scales), the
    slots at or past len_b empty, every table entry past ceil(len_b / page) naming an empty page."""
    B, Nmax, _ = codes.shape
    max_pages = Nmax // page
    assert max_pages * page == Nmax
    live = [(b, i) for b in range(B) for i in range(-(-min(max(lens[b], 0), Nmax) // page))]
    P = len(live) + spare
    order = list(range(P))
    random.Random(seed).shuffle(order)
    pool = empty_pool(P, page)
    pc, ps = views(pool)
    bt = torch.empty(B, max_pages, dtype=torch.int32)
    empty = order[len(live):]
    for b in range(B):
        for i in range(max_pages):
            bt[b, i] = empty[(b + i) % spare]
    for (b, i), p in zip(live, order):
        bt[b, i] = p
        n = min(page, lens[b] - i * page)
        pc.view(torch.uint8)[p, :n] = codes[b, i * page:i * page + n].view(torch.uint8)
        ps[p, :n] = scales[b, i * page:i * page + n]
    return pool, bt


def bf16_pool(pool):
    """The codes of an FP8 pool as a bf16 pool [P,page,128] (exact; 0x7F becomes NaN): what mla_index_logits_paged_bf16 takes."""
    return views(pool)[0].float().to(BF).contiguous()


# ---------------------------------------------------------------------------------------------------- logits

def _gather(pool, bt, b, top, mode):
    """(codes fp64 [top,128], scales fp64 [top]) of the first `top` positions of sequence b; the scale as `mode` reads it."""
    P, page, _ = pool.shape
    codes, scales = views(pool)
    j = torch.arange(top)
    pg, r = bt[b].long()[j // page], j % page
    c = codes[pg, r].double()
    if mode == "no_scale":
        s = torch.ones(top, dtype=torch.float64)
    elif mode == "next_slot":
        s = scales[pg, (r + 1) % page].double()
    elif mode == "other_page":  # the offset a page of half the size (twice the size at page 16) would give, in the pool's flat bytes
        other = page // 2 if page > 16 else 2 * page
        words = pool.view(-1).view(torch.float32)
        s = words[((pg * ROW * page + D * other + 4 * r) // 4) % words.numel()].double()
    else:
        s = scales[pg, r].double()
    return c, s


def logits_ref(q, w, pool, bt, lens, ld, modes=("right",)):
    """({mode: ref fp64 [B,T,ld]}, bound fp64 [B,T,ld], vis): NaN / 0 at the positions at or past vis. The modes: "right" (the contract);
    the scale dropped; slot r + 1's scale (in the same page); the scale at the offset a page of another size would give; ReLU after the head
    sum; no ReLU. The bound is the right reading's."""
    B, T, Hi, _ = q.shape
    cap = min(bt.shape[1] * pool.shape[1], ld)
    vis = visible(lens, T, cap)
    refs = {m: torch.full((B, T, ld), NAN, dtype=torch.float64) for m in modes}
    bound = torch.zeros(B, T, ld, dtype=torch.float64)
    qd, wd = q.double(), w.double()
    for b in range(B):
        top = max(vis[b])
        if top <= 0:
            continue
        c, s = _gather(pool, bt, b, top, "right")
        assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(s).all()) and bool((s > 0).all())
        dots = torch.einsum("thd,jd->thj", qd[b], c)
        a = torch.einsum("th,thj->tj", wd[b].abs(), torch.einsum("thd,jd->thj", qd[b].abs(), c.abs())) * s
        inside = torch.einsum("th,thj->tj", wd[b], dots.clamp_min(0))
        plain = torch.einsum("th,thj->tj", wd[b], dots)
        for m in modes:
            if m == "relu_after":
                lg = (plain * s).clamp_min(0)
            elif m == "relu_none":
                lg = plain * s
            else:
                lg = inside * (s if m == "right" else _gather(pool, bt, b, top, m)[1])
            for t in range(T):
                n = max(vis[b][t], 0)
                refs[m][b, t, :n] = lg[t, :n]
        for t in range(T):
            n = max(vis[b][t], 0)
            bound[b, t, :n] = a[t, :n] * EPS_TERMS * 2.0 ** -23
    return refs, bound, vis


# ---------------------------------------------------------------------------------------------------- the parity cases

SMALL_LENS, SMALL_NMAX = [1, 15, 16, 17, 0, 255, 256, 257, 100], 512  # a sequence of length 0 between live ones
LONG_LENS, LONG_NMAX = [1023, 1024, -3, 1025, 2100, 300], 2304        # a negative length; one length above 2048; 2304 = 9 x 256
# (lens, Hi, T, page, ld or None for ld = Nmax, scale_pow2): every Hi, T and page of the issue, ld below, equal to and above the cache, ld % 4 != 0
PARITY = {
    "small-Hi1-T1-p16": ("small", 1, 1, 16, None, True),
    "small-Hi16-T3-p64": ("small", 16, 3, 64, None, False),
    "small-Hi17-T1-p256": ("small", 17, 1, 256, None, True),
    "small-Hi33-T3-p16": ("small", 33, 3, 16, None, False),
    "small-Hi64-T3-p64": ("small", 64, 3, 64, None, True),
    "small-ld100": ("small", 17, 3, 16, 100, True),      # below the cache
    "small-ld513": ("small", 17, 3, 64, 513, True),      # above it, ld % 4 = 1
    "small-ld5002": ("small", 16, 1, 16, 5002, False),   # far above it, ld % 4 = 2
    "long-Hi64-T1-p64": ("long", 64, 1, 64, None, True),
    "long-Hi17-T3-p256": ("long", 17, 3, 256, None, True),
    "long-Hi33-T1-p16": ("long", 33, 1, 16, 2303, False),  # ld % 4 = 3, one below the cache
}


def _keys(B, Nmax, seed):
    """bf16 [B,Nmax,128]: normal draws times a per-token magnitude 2^u, u uniform in [-4, 4]: neighbouring tokens have different scales."""
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** (torch.rand(B, Nmax, 1, generator=g) * 8 - 4)
    return (torch.randn(B, Nmax, D, generator=g) * mag).to(BF)


def _queries(B, T, Hi, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, Hi, D, generator=g).to(BF)
    w = (torch.randn(B, T, Hi, generator=g) * (Hi * D) ** -0.5).float()  # both signs
    return q, w


def quantised_pool(keys, page, lens, pow2, seed):
    B, Nmax, _ = keys.shape
    kc, ks = quantise_rows(keys.reshape(B * Nmax, D), pow2)
    return make_pool(kc.view(B, Nmax, D), ks.view(B, Nmax), page, lens, seed=seed)


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """(q, w, (pool, bt), lens, ld) of PARITY[name]."""
    which, Hi, T, page, ld, pow2 = PARITY[name]
    lens, Nmax = (SMALL_LENS, SMALL_NMAX) if which == "small" else (LONG_LENS, LONG_NMAX)
    seed = sorted(PARITY).index(name)
    q, w = _queries(len(lens), T, Hi, 300 + seed)
    return q, w, quantised_pool(_keys(len(lens), Nmax, 400 + seed), page, lens, pow2, seed), lens, ld or Nmax


@functools.lru_cache(maxsize=None)
def reference(name):
    """(ref, bound, vis) of parity_case(name), the right reading."""
    q, w, (pool, bt), lens, ld = parity_case(name)
    refs, bound, vis = logits_ref(q, w, pool, bt, lens, ld)
    return refs["right"], bound, vis


@functools.lru_cache(maxsize=None)
def exact_case(Hi=64, T=3, page=16, unit_scales=False):
    """Integer q in [-4, 4], integer codes in [-8, 8], integer weights in [-4, 4], scales 2^e with e in -3 ... 3 (or all 1): every partial sum
    is an integer below 128 x 32 x 4 x 64 = 2^20 and the scale shifts its exponent, so every logit is computed without rounding whatever the
    order."""
    g = torch.Generator().manual_seed(78)
    B = len(SMALL_LENS)
    q = torch.randint(-4, 5, (B, T, Hi, D), generator=g).to(BF)
    c = torch.randint(-8, 9, (B, SMALL_NMAX, D), generator=g).float().to(F8)
    w = torch.randint(-4, 5, (B, T, Hi), generator=g).float()
    s = 2.0 ** torch.randint(-3, 4, (B, SMALL_NMAX), generator=g).float()
    if unit_scales:
        s = torch.ones_like(s)
    return q, w, make_pool(c, s, page, SMALL_LENS, seed=5), SMALL_LENS, SMALL_NMAX


# ---------------------------------------------------------------------------------------------------- append problems

APPEND_PAGES = [16, 64, 256]
MARK_BYTE = 0xA5  # the pool's bytes before an append: as a code a finite value no test key quantises to in bulk, as a scale -2.9e-16


@functools.lru_cache(maxsize=None)
def append_problem(name, page):
    """mla_index_reference.append_problem(name) -- the twelve edges of the append's contract -- behind pages of `page` slots: the same
    recipe, with the lengths that are stated in pages scaled to this page. dict(page, P, bt, lens (after the append), cu, k_new, new); the
    keys have per-token magnitudes over 2^-4 ... 2^4."""
    assert name in ix.APPEND_CASES
    g = torch.Generator().manual_seed(150 + 16 * ix.APPEND_CASES.index(name) + page)
    max_pages, lead, trail = 8, 0, 0
    if name == "ragged":
        new, lens, lead, trail = [0, 1, 5, 40], [37, 1, 18, 100], 2, 3
    elif name in ("page32", "page128", "page256"):  # rows across one and two page edges, the first sequence's row at another slot each
        first = {"page32": 1, "page128": page // 2, "page256": page}[name]
        max_pages = 4
        new, lens = [1, page + 3, 2 * page, 7], [first, 2 * page + 1, 3 * page, page - 1]
    elif name == "empties":
        new, lens = [0, 3, 0, 0, 20, 0], [5, 3, 0, 9, 41, 128]
    elif name == "single":
        new, lens = [1], [17]
    elif name == "b37":
        new = [0] * 37
        lens = [(7 * b) % 100 for b in range(37)]
        for b, t in ((0, 2), (13, 1), (18, 19), (35, 4), (36, 1)):
            new[b], lens[b] = t, max(lens[b], t)
    elif name == "slack":
        new, lens, lead, trail = [4, 17], [20, 17], 5, 9
    elif name == "short_len":
        new, lens = [5, 6, 3], [3, 0, 3]
    elif name == "past_nmax":
        new, lens = [6, 4, 2], [max_pages * page + 3, max_pages * page, max_pages * page + 2]
    elif name == "bad_entries":  # -1 under the last ten tokens of sequence 0 (its second page), P under the last four of sequence 1 (its third)
        new, lens = [20, 20, 3], [page + 10, 2 * page + 4, 3]
    else:  # cu_outside
        new, lens = [4, 6], [10, 30]
    B = len(new)
    cu = [lead]
    for t in new:
        cu.append(cu[-1] + t)
    total_q = cu[-1] + trail
    if name == "cu_outside":
        cu[0], cu[-1] = -3, total_q + 5
    P = B * max_pages + 2
    bt = torch.randperm(P, generator=g)[:B * max_pages].to(torch.int32).view(B, max_pages)
    if name == "bad_entries":
        bt[0, 1], bt[1, 2] = -1, P
    mag = 2.0 ** (torch.rand(max(total_q, 1), 1, generator=g) * 8 - 4)
    k_new = (torch.randn(max(total_q, 1), D, generator=g) * mag).to(BF)
    return dict(page=page, P=P, bt=bt, lens=lens, cu=cu, k_new=k_new, new=new)


def marked_pool(P, page):
    return torch.full((P, page, ROW), MARK_BYTE, dtype=torch.uint8)


def special_rows():
    """bf16 [6,128]: an all-zero key; a key of +-0 only; keys whose amax stands at a negative and at a positive element with +-0 around it;
    a key whose amax / 448 is a power of two (amax 448 x 2^-3); a key below the 1e-4 floor."""
    k = torch.zeros(6, D, dtype=BF)
    k[1, ::2] = -0.0
    k[2, 5], k[2, 6], k[2, 7], k[2, 9] = -3.5, 0.0, -0.0, 1.25
    k[3, 100], k[3, 0], k[3, 1], k[3, 127] = 3.5, -0.0, 0.0, -1.25
    k[4, 3], k[4, 4], k[4, 64] = 56.0, -7.0, 0.4375
    k[5, 1], k[5, 2] = 3e-5, -1e-5
    return k


# ---------------------------------------------------------------------------------------------------- a pool whose bytes pass 2^32

LARGE_PAGE, LARGE_BASE, LARGE_BUF_BYTES = 16, 16, (8 << 30) + (64 << 10) + 16  # the buffer of tests/paged_large_pool.py, the view 16 bytes in
LARGE_PB = ROW * LARGE_PAGE     # 2112 bytes a page: no power of two, so a wrapped offset lands inside a page, not on its start
LARGE_POISON_BYTE = 0xFF        # an e4m3fn NaN as a code, a NaN as the fp32 scale 0xFFFFFFFF
LARGE_LOW_PAGES = 8             # pages 0 .. 7 always hold poison
LARGE_BOUNDS = (31, 32)         # bytes 2^31 (where a signed 32-bit offset turns negative; an element is a byte here) and 2^32


def large_pages():
    """P of the [P, 16, 132] view: the whole pages that fit behind LARGE_BASE."""
    return (LARGE_BUF_BYTES - LARGE_BASE) // LARGE_PB


def large_images(n):
    """The pages a kernel would touch for page n if it formed the byte offset n 2112 + off, 0 <= off < 2112, in 32 bits: the offsets
    (n 2112 + off) mod 2^32 run over [x, x + 2112) mod 2^32 with x = n 2112 mod 2^32, which lies in at most two neighbouring pages (a run
    that crosses 2^32 continues at page 0). Listed directly; empty when n 2112 + 2111 < 2^32 (nothing wraps)."""
    if (n + 1) * LARGE_PB <= 1 << 32:
        return []
    x = (n * LARGE_PB) % (1 << 32)
    return sorted({x // LARGE_PB, ((x + LARGE_PB - 1) % (1 << 32)) // LARGE_PB} - {n})


def large_plan(n_live, seed=0):
    """{"P", "must", "named" (n_live pages: must first, then a seeded shuffle of the rest), "poison" (sorted), "dead"}. must: page P - 1 and, for
    each of bytes 2^31 and 2^32, the page that holds that byte (b = 2^k // 2112), the page above it and the page below it. The other named
    pages are P - 2, P - 3, ... Poison: pages 0 .. 7, both neighbours of every named page that are not named themselves, and every wrap image
    of every named page; no named page is the image of another."""
    P = large_pages()
    must = [P - 1]
    for k in LARGE_BOUNDS:
        b = (1 << k) // LARGE_PB
        must += [b, b + 1, b - 1]
    assert n_live >= len(must) == 7
    named, shadow = [], set()
    for cand in must + list(range(P - 2, 0, -1)):
        if len(named) == n_live:
            break
        im = large_images(cand)
        if cand in named or cand in shadow or cand < LARGE_LOW_PAGES or any(i in named for i in im):
            assert cand not in must
            continue
        named.append(cand)
        shadow.update(im)
    assert len(named) == n_live and named[:7] == must
    poison = set(range(LARGE_LOW_PAGES)) | shadow
    for n in named:
        poison.update(m for m in (n - 1, n + 1) if 0 <= m < P)
    poison -= set(named)
    rest = named[7:]
    random.Random(seed).shuffle(rest)
    return {"P": P, "must": must, "named": must + rest, "poison": sorted(poison), "dead": 3}
