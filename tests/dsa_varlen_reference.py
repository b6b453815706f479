"""Helpers of the packed ("varlen") DSA step's tests (tests/test_dsa_varlen_surface.py, tests/test_gpu_dsa_varlen.py): the five
packed entries mla_index_logits_paged_varlen_bf16[_fp8], mla_index_topk_varlen, fa2_decode_paged_mla_sparse_varlen_bf16[_fp8].

No reference of its own and no tolerance of its own: a packed problem is cut into its sequences and each goes through the EXISTING reference
of the fixed-T entry with B = 1, T = T_b (mla_index_reference.logits_ref / topk_ref, mla_index_fp8_reference.logits_ref,
paged_mla_sparse_reference.decode_sparse, paged_mla_sparse_fp8_reference.decode_sparse), whose bounds then hold unchanged. Those modules are
imported, not edited.

The one new rule -- which sequence a packed row belongs to -- is modelled twice: find_row is the kernels' clamped binary search
(csrc/dsa_varlen_row.cuh), row_brute the definition (the largest b with clamped cu_q[b] <= r); the surface test holds one against the other.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools

import torch

import mla_index_fp8_reference as ix8
import mla_index_reference as ix
import paged_mla_fp8_reference as mf
import paged_mla_reference as ml
import paged_mla_sparse_fp8_reference as sp8
import paged_mla_sparse_reference as sp

BF = torch.bfloat16
NAN, NEG_INF = float("nan"), float("-inf")
DC, DK, D = sp.DC, sp.DK, ix.D


# ---------------------------------------------------------------------------------------------------- the packed rows

def clamped(cu, total_q):
    """(c, Ts): the offsets clamped to [0, total_q] and T_b = max(c[b + 1] - c[b], 0)."""
    c = [min(max(int(x), 0), total_q) for x in cu]
    return c, [max(c[b + 1] - c[b], 0) for b in range(len(c) - 1)]


def find_row(cu, total_q, r):
    """(b, t, T_b) of packed row r, or None for a row of no sequence: the kernels' search, step for step."""
    c, _ = clamped(cu, total_q)
    lo, hi = 0, len(cu) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if c[mid] <= r:
            lo = mid + 1
        else:
            hi = mid
    b = lo - 1
    if b < 0:
        return None
    T = max(c[b + 1] - c[b], 0)
    t = r - c[b]
    return (b, t, T) if t < T else None


def row_brute(cu, total_q, r):
    """The definition: the largest b in [0, B) with clamped cu_q[b] <= r; no sequence if there is none or t >= T_b."""
    c, Ts = clamped(cu, total_q)
    bs = [b for b in range(len(cu) - 1) if c[b] <= r]
    if not bs:
        return None
    b = bs[-1]
    return (b, r - c[b], Ts[b]) if r - c[b] < Ts[b] else None


def rows(cu, total_q):
    """[find_row(r) for every packed row]."""
    return [find_row(cu, total_q, r) for r in range(total_q)]


def sequences(cu, total_q):
    """[(b, c0, T_b)] of the sequences with a token, for well-formed offsets."""
    c, Ts = clamped(cu, total_q)
    return [(b, c[b], Ts[b]) for b in range(len(Ts)) if Ts[b] > 0]


def uniform_cu(B, T):
    return [b * T for b in range(B + 1)]


# ---------------------------------------------------------------------------------------------------- per-sequence references

def logits_ref(q, w, pool, bt, lens, cu, ld, fp8=False):
    """(ref fp64 [total_q,ld], bound fp64 [total_q,ld]): NaN / 0 wherever the packed entry writes nothing -- at or past vis, and the whole
    row of a row of no sequence. Each sequence through the fixed-T reference with B = 1, T = T_b."""
    total_q = q.shape[0]
    ref = torch.full((total_q, ld), NAN, dtype=torch.float64)
    bound = torch.zeros(total_q, ld, dtype=torch.float64)
    for b, c0, T in sequences(cu, total_q):
        args = (q[c0:c0 + T][None], w[c0:c0 + T][None], pool, bt[b:b + 1], [lens[b]], ld)
        if fp8:
            refs, bd, _ = ix8.logits_ref(*args)
            r = refs["right"]
        else:
            r, bd, _ = ix.logits_ref(*args)
        ref[c0:c0 + T], bound[c0:c0 + T] = r[0], bd[0]
    return ref, bound


def topk_ref(logits, lens, cu, topk):
    """int32 [total_q,topk]: mla_index_reference.topk_ref per sequence; a row of no sequence all -1."""
    total_q = logits.shape[0]
    out = torch.full((total_q, topk), -1, dtype=torch.int32)
    for b, c0, T in sequences(cu, total_q):
        out[c0:c0 + T] = ix.topk_ref(logits[c0:c0 + T][None], [lens[b]], topk)[0]
    return out


def sparse_ref(q, pool, bt, lens, cu, indices, scale, kv_scale=None):
    """(O [total_q,Hq,512], LSE [total_q,Hq], O_emul), fp64: the fixed-T sparse reference per sequence (the FP8 one with kv_scale); a row of
    no sequence O = 0, LSE = -inf."""
    total_q, Hq, _ = q.shape
    O = torch.zeros(total_q, Hq, DC, dtype=torch.float64)
    L = torch.full((total_q, Hq), NEG_INF, dtype=torch.float64)
    E = torch.zeros(total_q, Hq, DC, dtype=torch.float64)
    for b, c0, T in sequences(cu, total_q):
        a = (q[c0:c0 + T][None], pool, bt[b:b + 1], [lens[b]], indices[c0:c0 + T][None])
        o, l, e = sp.decode_sparse(*a, scale) if kv_scale is None else sp8.decode_sparse(*a, kv_scale, scale)
        O[c0:c0 + T], L[c0:c0 + T], E[c0:c0 + T] = o[0], l[0], e[0]
    return O, L, E


def vis_rows(lens, cu, total_q, cap):
    """vis(r) per packed row, None for a row of no sequence."""
    out = []
    for row in rows(cu, total_q):
        out.append(None if row is None else min(max(int(lens[row[0]]), 0), cap) - (row[2] - 1 - row[1]))
    return out


# ---------------------------------------------------------------------------------------------------- the ragged batch

# B = 7, T_b = (0, 1, 3, 0, 70, 2, 0) with two rows in front of cu_q[0] and three behind cu_q[B]: the smallest batch that takes every branch
# of the search -- empty sequences at the front, in the middle and at the back, rows of no sequence at both ends
RAGGED_T = (0, 1, 3, 0, 70, 2, 0)
RAGGED_FRONT, RAGGED_BACK = 2, 3
RAGGED_CU = [RAGGED_FRONT + sum(RAGGED_T[:b]) for b in range(len(RAGGED_T) + 1)]
RAGGED_TOTAL = RAGGED_CU[-1] + RAGGED_BACK
assert RAGGED_TOTAL == 81 and RAGGED_CU == [2, 2, 3, 6, 6, 76, 78, 78]
# vis per sequence: b1 1023 (one below the logits kernel's chunk edge); b2 0, 1, 2 (a length shorter than T_b: vis <= 0, then 1); b4
# 31 ... 100 (every 16-key block edge from 32 to 96, and the causal edge crosses the 64-slot step of the sparse kernel); b5 1024, 1025 (the
# chunk edge and one past it); the sequences without a token hold lengths that must not matter
RAGGED_LENS = [500, 1023, 2, 0, 100, 1025, 7]
PAGE, MAX_PAGES = 16, 128
NMAX = PAGE * MAX_PAGES
assert NMAX == 2048
SINGLE_CU, SINGLE_LENS, SINGLE_TOTAL = [1, 4], [40], 6          # B = 1: T_0 = 3 with one row in front and two behind
EMPTY_CU, EMPTY_LENS, EMPTY_TOTAL = [0, 0], [40], 3             # a single sequence without a token: every row belongs to none
MALFORMED = {"decreasing": [40, 30, 60, 20, 10, 81, 5, 0], "negative": [-5, -1, 3, 6, 6, 76, 78, 78],
             "too_large": [2, 2, 3, 6, 6, 76, 500, 1 << 30]}
UNIFORM_BT = [(5, 1), (3, 4), (2, 70)]


def _g(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def index_keys(B):
    return torch.randn(B, NMAX, D, generator=_g(31 + B)).to(BF)


@functools.lru_cache(maxsize=None)
def index_pool(lens, fp8=False):
    """(pool, block_table) of the index keys of `lens` (a tuple): bf16 [P,16,128] with NaN in every unlisted row, or the FP8 pool uint8
    [P,16,132] with NaN codes and NaN scales there."""
    keys = index_keys(len(lens))
    if fp8:
        return ix8.quantised_pool(keys, PAGE, list(lens), True, seed=5)
    return ix.make_pool(keys, PAGE, list(lens), seed=5)


@functools.lru_cache(maxsize=None)
def index_queries(total_q, Hi, nan_rows=()):
    """(q_idx bf16 [total_q,Hi,128], weights fp32 [total_q,Hi]); the rows in nan_rows are NaN in both."""
    g = _g(1000 + 7 * total_q + Hi)
    q = torch.randn(total_q, Hi, D, generator=g).to(BF)
    w = (torch.randn(total_q, Hi, generator=g) * (Hi * D) ** -0.5).float()
    for r in nan_rows:
        q[r], w[r] = NAN, NAN
    return q, w


@functools.lru_cache(maxsize=None)
def latent_dense(B):
    return (torch.randn(B, NMAX, DK, generator=_g(77 + B)) * sp.SCALE).to(BF)


KV_SCALE = 2.0 ** -8


@functools.lru_cache(maxsize=None)
def latent_pool(lens, fp8=False):
    """(pool, block_table) of the latent rows of `lens`: bf16 [P,16,576] with NaN in every unlisted row, or e4m3fn codes quantised at
    KV_SCALE with NaN bytes there."""
    dense = latent_dense(len(lens))
    if fp8:
        return mf.make_pool(mf.quantize(dense, KV_SCALE), PAGE, list(lens), seed=9)
    return ml.make_pool(dense, PAGE, list(lens), seed=9)


@functools.lru_cache(maxsize=None)
def latent_queries(total_q, Hq, nan_rows=(), mult=1):
    q = (torch.randn(total_q, Hq, DK, generator=_g(2000 + 3 * total_q + Hq)) * sp.SCALE).to(BF)
    q = ml.times(q, mult) if mult != 1 else q
    for r in nan_rows:
        q[r] = NAN
    return q


@functools.lru_cache(maxsize=None)
def packed_indices(lens, cu, total_q, topk, seed=0):
    """int32 [total_q,topk]: per sequence paged_mla_sparse_reference.sample_indices at T = T_b (distinct visible positions scattered over
    the slots with empty slots between them); a row of no sequence lists 0 ... topk - 1, positions that would be valid in any sequence long
    enough -- a kernel that served the row would read pool rows. Past topk 256 a list holds at most 160 valid slots, scattered over all its
    splits: the fp64 reference and its emulation stay quick."""
    out = torch.arange(topk, dtype=torch.int32).repeat(total_q, 1)
    for b, c0, T in sequences(list(cu), total_q):
        out[c0:c0 + T] = sp.sample_indices([lens[b]], T, NMAX, topk, seed=seed + 13 * b + topk, want=160 if topk > 256 else None)[0]
    return out


def no_sequence_rows(cu, total_q):
    return tuple(r for r, row in enumerate(rows(list(cu), total_q)) if row is None)
