"""Helpers of the tests of the sparse multi-head latent attention decode over a paged latent cache held in FP8
(tests/test_paged_mla_sparse_fp8_surface.py, tests/test_gpu_paged_mla_sparse_fp8*.py): the fp64 reference and the bf16 emulation
of cuda_learn_notes_amd.fa2_decode_paged_mla_sparse_bf16_fp8 and the cases of the GPU tests. Built from paged_mla_sparse_reference (the lists,
the validity rule, the builders of the cases, the plan rule) and paged_mla_fp8_reference (quantize, the pools of codes, emul_rows); nothing is
free-standing.

The pool is e4m3fn [P, page, 576] with ONE fp32 kv_scale: value = e4m3(code) * kv_scale. Query token (b, t) attends to the valid slots of
indices[b, t], in slot order, exactly as in paged_mla_sparse_reference.decode_sparse:
  fp64 reference   on the rows of the pool dequantised in float64.
  emulation        paged_mla_fp8_reference.emul_rows on the gathered CODES taken as bf16 values, all of them visible.
At kv_scale 2^-8 both equal paged_mla_sparse_reference.decode_sparse on the pool dequantised to bf16, and on the dense list
paged_mla_fp8_reference.decode (asserted by the surface test). on_scores / on_o: how many times kv_scale enters the scores / O (1 and 1: the
entry; anything else: a mistake the surface test shows the family's bound can see on every parity case). The criteria are the family's, no
new tolerance: O within paged_bf16_reference.o_bound(emul, ref), LSE within decode_reference.lse_tol, -inf rows and zero rows exactly.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools

import torch

import paged_mla_fp8_reference as mf
import paged_mla_reference as ml
import paged_mla_sparse_reference as sp
import paged_softcap_reference as cr

BF, F8 = torch.bfloat16, mf.F8
DC, DR, DK, SCALE = ml.DC, ml.DR, ml.DK, ml.SCALE
NEG_INF = float("-inf")
NAN_BYTE = mf.NAN_BYTE
KV_SCALES = mf.KV_SCALES
WRONG = ((0, 1), (2, 1), (1, 0), (1, 2))  # (on_scores, on_o): kv_scale dropped from the scores, twice there, dropped from O, twice there


def decode_sparse(q, pool, block_table, lens, indices, kv_scale, scale, on_scores=1, on_o=1, emul=True):
    """(O [B,T,Hq,512], LSE [B,T,Hq], O_emul [B,T,Hq,512]), all fp64: q bf16 [B,T,Hq,576], pool e4m3fn [P,page,576], indices int [B,T,topk],
    kv_scale a Python float (taken as fp32). emul=False: O_emul stays zeros (the mistakes need only O and LSE)."""
    B, T, Hq, dk = q.shape
    page = pool.shape[1]
    vis = sp.visible(lens, T, block_table.shape[1] * page)
    x = cr.f32(scale)
    kvs = float(torch.tensor(kv_scale, dtype=torch.float32))
    codes = pool.to(BF)  # every e4m3 value is a bf16 value
    O = torch.zeros(B, T, Hq, DC, dtype=torch.float64)
    L = torch.full((B, T, Hq), NEG_INF, dtype=torch.float64)
    E = torch.zeros(B, T, Hq, DC, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            pos = [p for _, p in sp.valid_slots(indices[b, t], vis[b][t])]
            if not pos:
                continue
            pt = torch.tensor(pos)
            c = codes[block_table[b, pt // page].long(), pt % page]  # [n, 576] in slot order; only entries of valid positions are followed
            rows = c.double() * kvs                                  # the pool dequantised in float64
            s = q[b, t].double() @ rows.T * x * kvs ** (on_scores - 1)
            lse = torch.logsumexp(s, dim=-1)
            O[b, t] = torch.exp(s - lse[:, None]) @ rows[:, :DC] * kvs ** (on_o - 1)
            L[b, t] = lse
            if emul:
                E[b, t] = mf.emul_rows(q[b, t], c, [len(pos)] * Hq, scale, kv_scale, DC, on_scores, on_o)
    return O, L, E


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test

ONE_TH, ONE_TOPK, ONE_PAGES, SPLIT_TH = sp.ONE_TH, sp.ONE_TOPK, (16, 64), sp.SPLIT_TH

# The scores of the family's data are about 0.01: a softmax too flat for O to tell kv_scale twice in the scores from once. As DESIGN 4.4.21
# did for the softmax scale, q is multiplied by a power of two (exact in bf16): the smallest at which every mistake of WRONG lies SENSITIVITY x
# o_bound from the true reference, found per case on the CPU by find_q_mult() and asserted by the surface test. Of the 172 parity cases
# (160 of one split, 12 of several) all but 26 needed one: the smallest was 16 for 4 cases, 32 for 24, 64 for 100 and 128 for 12 (Hq 1 at
# topk >= 63), at either kv_scale alike; the several-splits cases needed 16 (Hq 16) and 32. One multiplier per kind of case, the largest any
# of its cases needed, keeps the cases few; that it holds the margin on EVERY case is what the surface test asserts.
# At topk 1 a token has one key, its weight is 1 and O cannot depend on the scores at all: there the two mistakes in the scores are held
# against SENSITIVITY x the LSE tolerance instead, the criterion that would catch them on the GPU (26 cases met it at 1, 6 at 2).
Q_MULT_ONE = {2.0 ** -8: 128, 0.003: 128}
Q_MULT_SPLIT = {2.0 ** -8: 32, 0.003: 32}


def _quantised(dense, page, lens, seed, kv_scale):
    return mf.make_pool(mf.quantize(dense, kv_scale), page, lens, seed=seed)


@functools.lru_cache(maxsize=None)
def one_case(T, Hq, page, kv_scale):
    """case 1: (q x Q_MULT_ONE, lens, (pool of codes, block_table)): paged_mla_sparse_reference.one_case's q, lengths and dense rows, the rows
    quantised on the CPU at kv_scale, the same pages in the same places, the dead pages NaN bytes."""
    q, lens, _ = sp.one_case(T, Hq, page)
    return ml.times(q, Q_MULT_ONE[kv_scale]), lens, _quantised(sp._dense(len(lens), sp.ONE_NMAX), page, lens, T + Hq + 1, kv_scale)


one_indices = sp.one_indices


@functools.lru_cache(maxsize=None)
def split_case(T, Hq, kv_scale):
    """case 2: (q x Q_MULT_SPLIT, lens, (pool of codes, block_table)): paged_mla_sparse_reference.split_case quantised; topk 2048."""
    q, lens, _ = sp.split_case(T, Hq)
    dense = sp._dense(len(lens), sp.SPLIT_PAGE * sp.SPLIT_MAX_PAGES)
    return ml.times(q, Q_MULT_SPLIT[kv_scale]), lens, _quantised(dense, sp.SPLIT_PAGE, lens, Hq + 1, kv_scale)


split_indices = sp.split_indices


@functools.lru_cache(maxsize=None)
def scale_case(kv_scale):
    """The case of the tests at another softmax scale: (q, lens, (pool, block_table), indices) of split_case(2, 40) with the valid slots of
    the length-100 sequence in the last chunk, q x paged_mla_reference.Q_MULT in all, as the siblings' scale_case."""
    q, lens, pool = split_case(2, 40, kv_scale)
    return ml.times(q, ml.Q_MULT // Q_MULT_SPLIT[kv_scale]), lens, pool, split_indices(2, 40, True)


@functools.lru_cache(maxsize=None)
def many_case(T, Hq, kv_scale):
    """case 7: paged_mla_sparse_reference.many_case quantised: (q, lens, (pool of codes, block_table), indices)."""
    q, lens, _, idx = sp.many_case(T, Hq)
    dense = sp._dense(len(lens), sp.MANY_PAGE * sp.MANY_MAX_PAGES)
    return q, lens, _quantised(dense, sp.MANY_PAGE, lens, T, kv_scale), idx


def parity_cases():
    """Every parity case of the GPU file as (what, q, lens, (pool, block_table), indices, kv_scale)."""
    for kv_scale in KV_SCALES:
        for (T, Hq) in ONE_TH:
            for page in ONE_PAGES:
                for topk in ONE_TOPK:
                    yield ("one", T, Hq, page, topk, kv_scale), *one_case(T, Hq, page, kv_scale), one_indices(T, Hq, page, topk), kv_scale
        for (T, Hq) in SPLIT_TH:
            for last in (False, True):
                yield ("split", T, Hq, sp.SPLIT_PAGE, last, kv_scale), *split_case(T, Hq, kv_scale), split_indices(T, Hq, last), kv_scale


def deq_bf16(pool, bt, lens, kv_scale):
    """The pool dequantised to bf16 (exact at a power-of-two scale), the dead pages zero: test_gpu_paged_mla_fp8.deq_bf16."""
    x = mf.dequantize(mf.zero_dead_pages(pool, bt, lens), kv_scale, torch.float64)
    assert torch.equal(x.to(BF).double(), x)
    return x.to(BF)


# ---------------------------------------------------------------------------------------------------- the bound sees where kv_scale goes

def margins(q, pool, bt, lens, idx, kv_scale):
    """[(mistake, distance, what it must reach)] for the four mistakes of WRONG: max |O_wrong - O| against SENSITIVITY x o_bound(emul, O); where
    no token has more than one valid slot and the mistake is in the scores, max |LSE_wrong - LSE| against SENSITIVITY x lse_tol."""
    import decode_reference as dr
    import paged_bf16_reference as br
    ro, rl, emul = decode_sparse(q, pool, bt, lens, idx, kv_scale, SCALE)
    fin = torch.isfinite(rl)
    assert bool(fin.any())
    vis = sp.visible(lens, q.shape[1], bt.shape[1] * pool.shape[1])
    single = max(len(sp.valid_slots(idx[b, t], vis[b][t])) for b in range(q.shape[0]) for t in range(q.shape[1])) <= 1
    out = []
    for on_scores, on_o in WRONG:
        wo, wl, _ = decode_sparse(q, pool, bt, lens, idx, kv_scale, SCALE, on_scores, on_o, emul=False)
        if single and on_o == 1:
            out.append(((on_scores, on_o), float((wl[fin] - rl[fin]).abs().max()), ml.SENSITIVITY * dr.lse_tol(rl)))
        else:
            out.append(((on_scores, on_o), float((wo - ro).abs().max()), ml.SENSITIVITY * br.o_bound(emul, ro)))
    return out


def find_q_mult(q, pool, bt, lens, idx, kv_scale, top=2 ** 12):
    """The smallest power of two m at which every margin of q x m holds (how the Q_MULT tables above were found)."""
    m = 1
    while m <= top:
        if all(d >= need for _, d, need in margins(ml.times(q, m), pool, bt, lens, idx, kv_scale)):
            return m
        m *= 2
    return None
