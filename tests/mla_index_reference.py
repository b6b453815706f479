"""Helpers of the DSA indexer tests (tests/test_mla_index_surface.py, tests/test_gpu_mla_index.py): the fp64 reference of
cuda_learn_notes_amd.mla_index_logits_paged_bf16 with its derived bound, the exact reference of mla_index_topk, the reference of
kv_append_paged_index_bf16, the case builders, and a torch model of the top-k kernel's three steps with named faults (topk_model), which
the surface test uses to prove that the long-row cases of tests/test_gpu_mla_index_long_rows.py bite.

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
    """The pool after kv_append_paged_index_bf16, to the contract of csrc/kv_append_paged_index_bf16.cuh and include/cln_amd_ext.h: the offsets
    clamped to [0, total_q], T_b = max(c[b + 1] - c[b], 0), packed row c[b] + i at position lens_after[b] - T_b + i, bit for bit; a token
    with pos < 0 or pos >= Nmax writes nothing, nor does one whose table entry lies outside [0, P)."""
    out = pool.clone()
    P, page = pool.shape[:2]
    Nmax = bt.shape[1] * page
    c, Ts = append_clamped(cu, k_new.shape[0])
    for b in range(len(lens_after)):
        for i in range(Ts[b]):
            pos = lens_after[b] - Ts[b] + i
            if 0 <= pos < Nmax and 0 <= int(bt[b, pos // page]) < P:
                out[int(bt[b, pos // page]), pos % page] = k_new[c[b] + i]
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


# ---------------------------------------------------------------------------------------------------- the logits cases of every head-block count

ONE_HT_MORE = [(32, 3), (33, 3), (48, 1), (49, 1), (63, 3)]  # NHB = ceil(Hi / 16) = 2, 3, 3, 4, 4: a full second block, both ends of NHB = 3, 4
PAGED_HT = (17, 8)
PAGED_NMAX = {32: 320, 128: 512, 256: 4096}  # make_pool wants Nmax divisible by the page
NEG_LENS = [65, -5, 257, 0, 17]
ALIGN_LDS = [4101, 4102, 4103]  # ld mod 4 = 1, 2, 3: rows at every multiple of 4 bytes past a 16-byte boundary


@functools.lru_cache(maxsize=None)
def paged_case(page, Hi=PAGED_HT[0], T=PAGED_HT[1]):
    """one_case's lengths behind pages of 32, 128 or 256 rows (page 256: the sixteen table entries of a wave are one entry); ld = Nmax."""
    Nmax = PAGED_NMAX[page]
    q, w = _queries(len(ONE_LENS), T, Hi, 100 * Hi + T + page)
    return q, w, make_pool(_keys(len(ONE_LENS), Nmax, 7), page, ONE_LENS, seed=Hi + T + page), ONE_LENS, Nmax


@functools.lru_cache(maxsize=None)
def long_case_paged(page):
    """long_case's queries, keys and lengths behind another page size."""
    Hi, T = LONG_HT
    q, w = _queries(len(LONG_LENS), T, Hi, 5)
    return q, w, make_pool(_keys(len(LONG_LENS), LONG_NMAX, 9), page, LONG_LENS, seed=2 + page), LONG_LENS, LONG_NMAX


@functools.lru_cache(maxsize=None)
def neg_case(Hi=17, T=3, page=16):
    """A sequence of length -5 between live ones: it has no visible position, its table row names NaN pages only."""
    q, w = _queries(len(NEG_LENS), T, Hi, 31)
    return q, w, make_pool(_keys(len(NEG_LENS), ONE_NMAX, 11), page, NEG_LENS, seed=6), NEG_LENS, ONE_NMAX


ROWS_LENS, ROWS_NMAX, ROWS_HI, ROWS_LD = [0, 2048, 300, 17, 2000], 2048, 17, 2 ** 30 + 1


@functools.lru_cache(maxsize=None)
def rows_case():
    """The problem of tests/test_gpu_mla_index_large_rows.py: T = 1, two chunks of 1024 keys, sequence 0 empty; ld = Nmax in the small run."""
    q, w = _queries(len(ROWS_LENS), 1, ROWS_HI, 41)
    return q, w, make_pool(_keys(len(ROWS_LENS), ROWS_NMAX, 12), 16, ROWS_LENS, seed=8), ROWS_LENS, ROWS_NMAX


@functools.lru_cache(maxsize=None)
def rows_topk_case(topk=64):
    """(logits fp32 [5,1,2048], lens): random eighths with ties, NaN at every j >= n; every row longer than topk has a list other than
    [0 ... topk - 1], so reading another row's (NaN) window instead of its own changes the answer."""
    g = torch.Generator().manual_seed(17)
    x = (torch.randint(-20, 21, (len(ROWS_LENS), 1, ROWS_NMAX), generator=g).float() / 8).contiguous()
    for b, n in enumerate(ROWS_LENS):
        x[b, 0, n:] = NAN
    return x, ROWS_LENS


def row_start_wraps(r, ld=ROWS_LD):
    """Where a 32-bit byte offset (mod 2^30 elements) and a 32-bit element offset (mod 2^32) would put the start of row r of an fp32 [*, ld]
    tensor; the true start is r ld."""
    return (r * ld) % 2 ** 30, (r * ld) % 2 ** 32


# ---------------------------------------------------------------------------------------------------- a model of the top-k kernel, with faults

WAVES = 16
FAULTS_HARMFUL = ["ties_last", "no_carry_gt", "no_carry_eq", "stale_counts", "stop_after_two_blocks"]
FAULTS_HARMLESS = ["break_late_by_one_block", "no_slot_clip"]
UNWRITTEN = -2  # a slot the model never wrote (the kernel writes every slot; a fault may not)


def key_map(x):
    """Step 1 of csrc/mla_index_topk.cuh on a fp32 tensor: int64 keys whose unsigned order is the order of the logits; -0 as +0."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    return torch.where((u & 0x80000000) != 0, u ^ 0xFFFFFFFF, u | 0x80000000)


def radix_select(keys, topk):
    """Step 2: (prefix, krem) after four passes of 8 bits from the top -- the key of the topk-th largest and how many of its ties are taken."""
    prefix, himask, krem = 0, 0, topk
    for shift in (24, 16, 8, 0):
        hist = torch.bincount((keys[(keys & himask) == prefix] >> shift) & 255, minlength=256).tolist()
        above = 0
        for d in range(255, -1, -1):
            if above < krem <= above + hist[d]:
                prefix, krem = prefix | (d << shift), krem - above
                break
            above += hist[d]
        else:
            raise AssertionError("no digit holds the k-th key")
        himask |= 255 << shift
    return prefix, krem


def _excl(x):
    return torch.cumsum(x, -1) - x


def topk_model(vals, topk, fault=None, block=SCAN_BLOCK):
    """Steps 1 - 3 of csrc/mla_index_topk.cuh on one row of n > topk fp32 values, in plain torch: the ordered pass in blocks of `block`
    positions, WAVES waves of block / WAVES consecutive positions each, the per-wave counts in tot[blk & 1], the carried run_gt / run_eq and
    the break. Returns (list int32 [topk], info): info has prefix, krem, blocks (the blocks the pass ran), nblocks, spill (the (slot, position)
    writes at slots >= topk, which land in the next row). fault: None, or one of FAULTS_HARMFUL + FAULTS_HARMLESS:
      ties_last                the last krem ties instead of the first
      no_carry_gt, no_carry_eq run = all instead of run += all: what the blocks in front of the previous one carried is dropped at the edge (two
                               blocks cannot show it: the carry into block 1 is block 0's count either way)
      stale_counts             block b >= 2 finds block b - 2's wave counts in its buffer (its own write is lost)
      stop_after_two_blocks    the pass ends behind block 1
      break_late_by_one_block  the break tests the carries of the block before
      no_slot_clip             no `slot < topk` in front of the store
    Why no_slot_clip is harmless on consistent data: a selected greater key has fewer than G greater keys before it (G all of them) and
    min(eq, krem) <= krem, a selected tie has eq < krem and at most G before it: slot <= G + krem - 1 = topk - 1 either way. The clip guards
    against a row that changes under the kernel, nothing else."""
    assert fault is None or fault in FAULTS_HARMFUL + FAULTS_HARMLESS
    n = vals.shape[0]
    assert n > topk and block % (4 * WAVES) == 0
    keys = key_map(vals)
    prefix, krem = radix_select(keys, topk)
    span = block // WAVES
    nblocks = -(-n // block)
    pad = torch.zeros(nblocks * block, dtype=torch.bool)
    G, E = pad.clone(), pad.clone()
    G[:n], E[:n] = keys > prefix, keys == prefix
    total_eq = int(E.sum())
    skip = total_eq - krem if fault == "ties_last" else 0  # the ties in front of the taken ones

    def taken(eq):  # the ties taken among the first eq
        return (eq - skip).clamp(0, krem) if torch.is_tensor(eq) else min(max(eq - skip, 0), krem)

    out = torch.full((topk,), UNWRITTEN, dtype=torch.int64)
    spill = []
    tot = torch.zeros(2, 2, WAVES, dtype=torch.int64)
    run_gt = run_eq = 0
    prev = (0, 0)
    blocks = 0
    for blk in range(nblocks):
        if fault == "stop_after_two_blocks" and blk == 2:
            break
        g = G[blk * block:(blk + 1) * block].view(WAVES, span).long()
        e = E[blk * block:(blk + 1) * block].view(WAVES, span).long()
        if not (fault == "stale_counts" and blk >= 2):
            tot[blk & 1, 0], tot[blk & 1, 1] = g.sum(1), e.sum(1)
        tg, te = tot[blk & 1, 0], tot[blk & 1, 1]
        gt = (run_gt + _excl(tg)[:, None] + _excl(g)).reshape(-1)
        eq = (run_eq + _excl(te)[:, None] + _excl(e)).reshape(-1)
        gf, ef = g.reshape(-1).bool(), e.reshape(-1).bool()
        slot = gt + taken(eq)
        sel = gf | (ef & (eq >= skip) & (eq - skip < krem))
        pos = torch.arange(blk * block, (blk + 1) * block)
        inside = sel & (slot < topk)
        out[slot[inside]] = pos[inside]
        if fault == "no_slot_clip":
            spill += list(zip(slot[sel & (slot >= topk)].tolist(), pos[sel & (slot >= topk)].tolist()))
        blocks += 1
        run_gt =(0 if fault == "no_carry_gt" else run_gt) + int(tg.sum())
        run_eq = (0 if fault == "no_carry_eq" else run_eq) + int(te.sum())
        test = prev if fault == "break_late_by_one_block" else (run_gt, run_eq)
        prev = (run_gt, run_eq)
        if test[0] + taken(test[1]) >= topk:
            break
    info = dict(prefix=prefix, krem=krem, blocks=blocks, nblocks=nblocks, spill=spill, keys=keys)
    return out.to(torch.int32), info


# ---------------------------------------------------------------------------------------------------- top-k on long rows

LONG_KINDS = ["late", "early", "straddle", "spread", "wave_edges"]
LONG_TOPK_LD = 20488
PROD_N = 131072  # the production row: 32 scan blocks


def long_ns(block=SCAN_BLOCK):
    """2 ... 6 scan blocks and ragged last blocks."""
    return [2 * block - 1, 2 * block, 2 * block + 1, 3 * block, 3 * block + 1, 4 * block, 4 * block + 1, 5 * block + 1]


def long_topks(block=SCAN_BLOCK):
    """1, 64, 2048, 4096, 4097, 6000 at the kernel's block of 4096; the same fractions of a smaller block for the brute-force comparison."""
    return [1, block // 64, block // 2, block, block + 1, block * 375 // 256]


def _pick(g, choices, count):
    return torch.tensor(choices)[torch.randint(0, len(choices), (count,), generator=g)]


def _subset(g, lo, hi, count):
    """count distinct positions of [lo, hi), sorted."""
    return (torch.randperm(hi - lo, generator=g)[:count] + lo).sort().values


HIGH, LOW = [2.0, 2.5, 3.0], [-1.0, -2.0, -3.0]


@functools.lru_cache(maxsize=None)
def long_row(kind, n, topk, block=SCAN_BLOCK):
    """(vals fp32 [n], facts) of one long row, or None where the recipe cannot hold (n <= topk: the dense list, covered elsewhere; straddle
    needs n > 3 block and topk >= 8). facts states the property the recipe claims; tests/test_mla_index_surface.py asserts every one
    against the model and the reference.
      late        a background below the threshold; every selected position at or behind facts["from"], the start of the last block (of
                  the last blocks that together hold more than topk positions, where the last one is too short), position n - 1 selected
      early       every selected position in front of facts["to"] = block ceil(topk / block): in block 0, for topk > block in blocks 0 and 1
      straddle    the threshold's ties: facts["e"] in block 0, as many in block 1, then every position from 2 block to n - 1 that holds no
                  greater key; facts["g"] greater keys in each of blocks 0, 1, 2 and none behind: the last tie taken lies inside block 2
      spread      the heavy ties of topk_case's "ties" (17 values): every block holds ties of the threshold and, once topk exceeds the
                  largest class (topk >= 2048 on the rows of up to six blocks), greater keys
      wave_edges  selected: the first and last position of every wave's span of block / 16 positions and positions = 3 mod 4, handed out
                  round-robin over the blocks until topk are found; where the row has fewer than topk of those, all of them and the first
                  ties (every other position holds the threshold)"""
    if n <= topk:
        return None
    g = torch.Generator().manual_seed(1000 * LONG_KINDS.index(kind) + 7 * n + topk)
    facts = {}
    if kind == "spread":
        x = torch.randint(-8, 9, (n,), generator=g).float() / 4
    elif kind in ("late", "early"):
        x = _pick(g, LOW, n)
        if kind == "late":
            lo = (n - 1) // block * block
            while n - lo <= topk:
                lo -= block
            win = torch.cat([_subset(g, lo, n - 1, topk - 1), torch.tensor([n - 1])])
            facts["from"] = lo
        else:
            hi = min(-(-topk // block) * block, n)
            win = _subset(g, 0, hi, topk)
            facts["to"] = hi
        x[win] = _pick(g, HIGH, topk)
        facts["selected"] = win
    elif kind == "straddle":
        ng, ne = max(1, topk // 6), max(1, topk // 12)
        cut = topk - 3 * ng - 2 * ne  # the ties taken in block 2
        if n <= 3 * block or topk < 8 or not 0 < cut < block - ng - 1:
            return None
        x = _pick(g, LOW, n)
        x[2 * block:] = 1.0
        for blk in range(3):  # block 2: at least half of its greater keys in front of the last tie taken, the others anywhere
            p = _subset(g, blk * block, (blk + 1) * block, ng + ne) if blk < 2 else torch.cat(
                [_subset(g, 2 * block, 2 * block + cut, ng - ng // 2), _subset(g, 2 * block + cut, 3 * block, ng // 2)])
            p = p[torch.randperm(len(p), generator=g)]
            x[p[:ng]] = _pick(g, HIGH, ng)
            x[p[ng:]] = 1.0
        facts.update(g=ng, e=ne, cut=cut)
    else:
        span = block // WAVES
        p = torch.arange(n)
        edge = (p % span == 0) | (p % span == span - 1)
        cand = p[edge | (p % 4 == 3)]
        order = sorted(cand.tolist(), key=lambda c: (0 if c % span in (0, span - 1) else 1, c % block, c // block))
        if len(order) >= topk:
            win = torch.tensor(sorted(order[:topk]))
            x = _pick(g, LOW, n)
            x[win] = _pick(g, HIGH, topk)
        else:
            x = torch.full((n,), 1.0)
            x[cand] = _pick(g, HIGH[1:], len(cand))
            rest = p[x == 1.0][:topk - len(cand)]
            win = torch.cat([cand, rest]).sort().values
        facts["selected"] = win
        facts["candidates"] = len(order)
    return x.float().contiguous(), facts


def long_logits(kind, n, topk, ld=LONG_TOPK_LD):
    """(logits fp32 [1,1,ld], [n]) of long_row, NaN at every j >= n; None where long_row is."""
    row = long_row(kind, n, topk)
    if row is None:
        return None
    x = torch.full((1, 1, ld), NAN)
    x[0, 0, :n] = row[0]
    return x, [n]


def old_topk_rows():
    """Every (row, topk) of topk_case with n > topk: the top-k cases from before the long rows (n <= 5000)."""
    for topk in TOPKS:
        for kind in VALUE_SETS:
            logits, ns = topk_case(topk, kind)
            for b, n in enumerate(ns):
                if n > topk:
                    yield logits[b, 0, :n], topk, (topk, kind, n)


# ---------------------------------------------------------------------------------------------------- rows at every 4-byte residue

ALIGN_B, ALIGN_T = 2, 3
ALIGN_KINDS = ["ties", "special"]


def align_lens(ld):
    """Two sets of lengths: between them n = 4097, 4100 and ld occur (n = min(len, ld) - (T - 1 - t))."""
    return [[ld + 5, 4099], [4100, ld]]


def row_residues(ld, base=0, rows=ALIGN_B * ALIGN_T):
    """The byte residues mod 16 of the starts of the rows of an fp32 [*, ld] tensor whose first byte is at `base`."""
    return [(base + 4 * r * ld) % 16 for r in range(rows)]


@functools.lru_cache(maxsize=None)
def align_case(ld, kind, which):
    """(logits fp32 [2,3,ld], lens): NaN at every j >= n(b, t)."""
    lens = align_lens(ld)[which]
    g = torch.Generator().manual_seed(ld + 3 * which + ALIGN_KINDS.index(kind))
    if kind == "ties":
        x = torch.randint(-8, 9, (ALIGN_B, ALIGN_T, ld), generator=g).float() / 4
    else:
        pick = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-45, -1e-45, 1e-40, -3e-39, 1.0, -1.0, 3.5, -2.5, 1e38, -1e38])
        x = pick[torch.randint(0, len(pick), (ALIGN_B, ALIGN_T, ld), generator=g)]
    x = x.clone()
    vis = visible(lens, ALIGN_T, ld)
    for b in range(ALIGN_B):
        for t in range(ALIGN_T):
            x[b, t, max(vis[b][t], 0):] = NAN
    return x.contiguous(), lens


# ---------------------------------------------------------------------------------------------------- append problems

MARK = 0x7FA5  # a bf16 NaN pattern no key holds: the pool's bytes before an append
APPEND_CASES = ["ragged", "page32", "page128", "page256", "empties", "single", "b37", "slack", "short_len", "past_nmax", "bad_entries",
                "cu_outside"]


@functools.lru_cache(maxsize=None)
def append_problem(name):
    """dict(page, P, bt int32 [B,max_pages], lens (after the append), cu, k_new bf16 [total_q,128], note) of one edge of
    kv_append_paged_index_bf16's contract. The table names distinct pages of a pool of P pages (two more than it needs); bad_entries puts
    -1 and P under live positions."""
    g = torch.Generator().manual_seed(50 + APPEND_CASES.index(name))
    page, max_pages, lead, trail = 16, 8, 0, 0
    if name == "ragged":  # the first append test's problem
        new, lens, lead, trail = [0, 1, 5, 40], [37, 1, 18, 100], 2, 3
    elif name in ("page32", "page128", "page256"):
        page = int(name[4:])
        max_pages = 4
        new, lens = [1, page + 3, 2 * page, 7], [1, 2 * page + 1, 3 * page, page - 1]  # rows across one and two page edges
    elif name == "empties":
        new = [0, 3, 0, 0, 20, 0]
        lens = [5, 3, 0, 9, 41, 128]
    elif name == "single":
        new, lens = [1], [17]
    elif name == "b37":  # the binary search at a B that is no power of two: five sequences with rows among 37
        new = [0] * 37
        lens = [(7 * b) % 100 for b in range(37)]
        for b, t in ((0, 2), (13, 1), (18, 19), (35, 4), (36, 1)):
            new[b], lens[b] = t, max(lens[b], t)
    elif name == "slack":  # packed rows of no sequence in front of cu[0] and behind cu[B]
        new, lens, lead, trail = [4, 17], [20, 17], 5, 9
    elif name == "short_len":  # seqlens[b] < T_b: the first T_b - seqlens[b] tokens have pos < 0
        new, lens = [5, 6, 3], [3, 0, 3]
    elif name == "past_nmax":  # seqlens[b] > Nmax: the tokens at pos >= Nmax write nothing
        new, lens = [6, 4, 2], [max_pages * page + 3, max_pages * page, max_pages * page + 2]
    elif name == "bad_entries":
        new, lens = [20, 20, 3], [40, 36, 3]
    else:  # cu_outside: cu[0] < 0 and cu[B] > total_q, clamped on the device to [0, total_q]
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
        bt[0, 1], bt[1, 2] = -1, P  # under positions 16 ... 31 of sequence 0 and 32 ... 47 of sequence 1
    k_new = torch.randn(max(total_q, 1), D, generator=g).to(BF)
    return dict(page=page, P=P, bt=bt, lens=lens, cu=cu, k_new=k_new, new=new)


def append_clamped(cu, total_q):
    """(clamped offsets, T_b) of the kernel header's contract: offsets clamped to [0, total_q], T_b = max(c[b + 1] - c[b], 0)."""
    c = [min(max(int(x), 0), total_q) for x in cu]
    return c, [max(c[b + 1] - c[b], 0) for b in range(len(c) - 1)]
