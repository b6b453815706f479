"""Helpers of the sparse multi-head latent attention tests (tests/test_paged_mla_sparse_surface.py, tests/test_gpu_paged_mla_sparse.py; DESIGN
4.4.20): the fp64 reference and the bf16 emulation of cuda_learn_notes_amd.fa2_decode_paged_mla_sparse_bf16, the plan rule restated, and the
cases of the GPU test.

The cache is paged_mla_reference's: one pool [P, page, 576] of latent rows behind a block table. Query token (b, t) brings a list
indices[b, t, 0 ... topk - 1] of logical token positions, shared by its heads. Slot k is valid iff
    0 <= idx < vis(b, t) = clamp(len_b, 0, max_pages page) - (T - 1 - t);
every other value is an empty slot. With V the valid slots in slot order:
    s_k = scale q . row(idx_k)[0:576],   O = softmax_V(s) row[:, 0:512],   LSE = ln sum_V exp(s_k);   V empty: O = 0, LSE = -inf.
A position listed twice is two keys. decode_sparse gathers the rows of V and hands them to paged_mla_reference.emul_rows with all of them
visible; with indices[b, t] = [0 ... vis - 1, -1 ...] it IS paged_mla_reference.decode, which the surface test asserts -- the reference is
not free-standing. The criteria are the family's, no new tolerance: O within paged_bf16_reference.o_bound(emul, ref), LSE within
decode_reference.lse_tol, -inf rows and zero rows exactly.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools
import random

import torch

import paged_mla_reference as ml
import paged_softcap_reference as cr

BF = torch.bfloat16
DC, DR, DK, SCALE = ml.DC, ml.DR, ml.DK, ml.SCALE
HEAD_GROUP, KEY_STEP, MAX_HQ = 64, 64, 128
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------------------- reference and emulation

def visible(lens, T, Nmax):
    """vis[b][t]: the dense entry's causal edge, may be <= 0."""
    return [[min(max(int(n), 0), Nmax) - (T - 1 - t) for t in range(T)] for n in lens]


def valid_slots(idx_row, vis):
    """The valid slots of one list, in slot order: [(slot, position)]."""
    return [(k, int(p)) for k, p in enumerate(idx_row.tolist()) if 0 <= p < vis]


def decode_sparse(q, pool, block_table, lens, indices, scale):
    """(O [B,T,Hq,512], LSE [B,T,Hq], O_emul [B,T,Hq,512]), all fp64: q bf16 [B,T,Hq,576], pool bf16 [P,page,576], indices int [B,T,topk]."""
    B, T, Hq, dk = q.shape
    page = pool.shape[1]
    vis = visible(lens, T, block_table.shape[1] * page)
    x = cr.f32(scale)
    O = torch.zeros(B, T, Hq, DC, dtype=torch.float64)
    L = torch.full((B, T, Hq), NEG_INF, dtype=torch.float64)
    E = torch.zeros(B, T, Hq, DC, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            pos = [p for _, p in valid_slots(indices[b, t], vis[b][t])]
            if not pos:
                continue
            pt = torch.tensor(pos)
            rows = pool[block_table[b, pt // page].long(), pt % page]  # [n, 576] in slot order; only entries of valid positions are followed
            s = q[b, t].double() @ rows.double().T * x
            lse = torch.logsumexp(s, dim=-1)
            O[b, t] = torch.exp(s - lse[:, None]) @ rows[:, :DC].double()
            L[b, t] = lse
            E[b, t] = ml.emul_rows(q[b, t], rows, [len(pos)] * Hq, scale, DC)
    return O, L, E


# ---------------------------------------------------------------------------------------------------- the plan, restated

def plan_rule(B, T, Hq, topk):
    """fa2d::split_plan(bk = B T ceil(Hq / 64), rows = B T Hq, Nmax = topk, unit = 64, D = 512): split the index slots until bk S reaches 1024
    workgroups but into chunks of at least 256 slots and at most 64 splits; chunk a multiple of 64; workspace rows S (512 + 2) 4 bytes when
    S > 1. Neither the context nor the page enters."""
    bk, want = B * T * (-(-Hq // HEAD_GROUP)), 1
    if bk < 1024 and topk > 256:
        want = min((1024 + bk - 1) // bk, topk // 256, 64)
    chunk = ((topk + want - 1) // want + KEY_STEP - 1) // KEY_STEP * KEY_STEP
    splits = (topk + chunk - 1) // chunk
    return splits, chunk, (B * T * Hq * splits * (DC + 2) * 4 if splits > 1 else 0)


# ---------------------------------------------------------------------------------------------------- index lists

def dense_indices(lens, T, Nmax, topk):
    """indices[b, t] = [0 ... vis - 1] then -1: the dense entry's key set."""
    vis = visible(lens, T, Nmax)
    out = torch.full((len(lens), T, topk), -1, dtype=torch.int32)
    for b in range(len(lens)):
        for t in range(T):
            n = max(vis[b][t], 0)
            assert n <= topk
            out[b, t, :n] = torch.arange(n, dtype=torch.int32)
    return out


def sample_indices(lens, T, Nmax, topk, seed, slot_range=None, want=None):
    """Per (b, t) a seeded random sample of min(vis, about 2/3 topk) distinct visible positions, unsorted, scattered over the slots (over
    slot_range[b] = (first, end) where given) with empty slots (-1) between them. want: the number of valid slots instead of 2/3 topk."""
    rnd = random.Random(seed)
    vis = visible(lens, T, Nmax)
    out = torch.full((len(lens), T, topk), -1, dtype=torch.int32)
    for b in range(len(lens)):
        first, end = slot_range[b] if slot_range and slot_range[b] else (0, topk)
        for t in range(T):
            n = min(max(vis[b][t], 0), want if want is not None else -(-2 * topk // 3), end - first)
            pos = rnd.sample(range(max(vis[b][t], 0)), n)
            slots = rnd.sample(range(first, end), n)
            for k, p in zip(slots, pos):
                out[b, t, k] = p
    return out


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test

ONE_TH = [(1, 1), (1, 16), (1, 17), (3, 5), (1, 64), (1, 65), (2, 128), (8, 3)]
ONE_TOPK = [1, 63, 64, 65, 200]
ONE_NMAX = ml.ONE_NMAX
SPLIT_LENS, SPLIT_PAGE, SPLIT_MAX_PAGES, SPLIT_TOPK = [4000, 2048, 300, 100, 0], 16, 256, 2048
SPLIT_TH = [(1, 16), (2, 40), (1, 128)]
MANY_TH, MANY_LENS, MANY_TOPK, MANY_PAGE, MANY_MAX_PAGES = [(33, 16), (70, 5)], [100, 20], 64, 16, 8


def _randn(shape, g):
    return (torch.randn(*shape, generator=g) * SCALE).to(BF)


@functools.lru_cache(maxsize=None)
def _dense(B, Nmax):
    return _randn((B, Nmax, DK), torch.Generator().manual_seed(11 * B + Nmax))


@functools.lru_cache(maxsize=None)
def one_case(T, Hq, page):
    """case 1: (q [8,T,Hq,576], lens, (pool, block_table)): paged_mla_reference's lengths at Nmax 320; one split for every topk <= 256."""
    lens = ml.ONE_LENS_SHORT if T == 8 else ml.ONE_LENS
    q = _randn((len(lens), T, Hq, DK), torch.Generator().manual_seed(100 * T + Hq + page + 1))
    return q, lens, ml.make_pool(_dense(len(lens), ONE_NMAX), page, lens, seed=T + Hq + 1)


@functools.lru_cache(maxsize=None)
def one_indices(T, Hq, page, topk):
    lens = ml.ONE_LENS_SHORT if T == 8 else ml.ONE_LENS
    return sample_indices(lens, T, ONE_NMAX, topk, seed=1000 * T + 10 * Hq + page + topk)


@functools.lru_cache(maxsize=None)
def split_case(T, Hq):
    """case 2: (q [5,T,Hq,576], lens, (pool, block_table)); Nmax 4096 at page 16, topk 2048: 8 splits of 256 slots."""
    q = _randn((len(SPLIT_LENS), T, Hq, DK), torch.Generator().manual_seed(1000 * T + Hq + 1))
    return q, SPLIT_LENS, ml.make_pool(_dense(len(SPLIT_LENS), SPLIT_PAGE * SPLIT_MAX_PAGES), SPLIT_PAGE, SPLIT_LENS, seed=Hq + 1)


@functools.lru_cache(maxsize=None)
def split_indices(T, Hq, last):
    """The lists of case 2. The length-100 sequence has all its valid slots in the first chunk (last = False) or in the last one (True): seven
    of its eight splits are empty."""
    rng = [None, None, None, (1792, 2048) if last else (0, 256), None]
    return sample_indices(SPLIT_LENS, T, SPLIT_PAGE * SPLIT_MAX_PAGES, SPLIT_TOPK, seed=7 * T + Hq + int(last), slot_range=rng)


@functools.lru_cache(maxsize=None)
def many_case(T, Hq):
    """case 8: many query tokens at lengths 100 and 20: the causal edge moves per token and the first tokens see fewer than topk keys, or none."""
    Nmax = MANY_PAGE * MANY_MAX_PAGES
    q = _randn((len(MANY_LENS), T, Hq, DK), torch.Generator().manual_seed(10 * T + Hq))
    pool = ml.make_pool(_dense(len(MANY_LENS), Nmax), MANY_PAGE, MANY_LENS, seed=T)
    return q, MANY_LENS, pool, sample_indices(MANY_LENS, T, Nmax, MANY_TOPK, seed=T + Hq)


@functools.lru_cache(maxsize=None)
def scale_case(T, Hq, split, scale):
    """paged_mla_reference.scale_case for the sparse entry: (q x Q_MULT, lens, (pool, block_table), indices, the reference at scale, the
    reference at SCALE) of one_case(T, Hq, 16) at topk 200 or split_case(T, Hq) at topk 2048."""
    q, lens, pool = split_case(T, Hq) if split else one_case(T, Hq, 16)
    idx = split_indices(T, Hq, True) if split else one_indices(T, Hq, 16, 200)
    q = ml.times(q, ml.Q_MULT)
    return q, lens, pool, idx, decode_sparse(q, *pool, lens, idx, scale), decode_sparse(q, *pool, lens, idx, SCALE)
