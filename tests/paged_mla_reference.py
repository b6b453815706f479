"""Helpers of the multi-head latent attention tests (tests/test_paged_mla_surface.py, tests/test_gpu_paged_mla.py): the fp64
reference and the bf16 emulation of cuda_learn_notes_amd.fa2_decode_paged_mla_bf16, the plan rule restated, and the cases of the GPU test.

The cache is one pool [P, page, dk] of latent rows; a row is the key with all its dk dims and the value with its first dv. A row r = t Hq + h of
sequence b sees the keys j < n = len_b - (T - 1 - t):
    s_j = scale q . row_j[0:dk],   O = softmax(s) row[:, 0:dv],   LSE = ln sum_j exp(s_j);   no key: O = 0, LSE = -inf.
dk and dv are parameters: with dv = dk = D and k_pages = v_pages = pool[:, None] this IS paged_softcap_reference.decode(..., W=None, sinks=None,
scale=s, cap=None), which the surface test asserts -- the reference is not free-standing.

The emulation follows paged_bf16_reference.emul_rows' six steps with the caller's scale, a dk-dim key and a dv-dim value: scores from the bf16
inputs in fp64, cast to fp32 and multiplied there by the fp32 number scale x log2(e); P = exp2 of the scores minus the row's final maximum; P
rounded to bf16; P V accumulated in fp64; divided by the fp32 row sum of the unrounded P; O rounded to bf16. The criteria are the family's, no new
tolerance: O within paged_bf16_reference.o_bound(emul, ref), LSE within decode_reference.lse_tol, -inf rows and zero rows exactly.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools
import math

import torch

import multi_decode_reference as mr
import paged_softcap_reference as cr

BF = torch.bfloat16
DC, DR, DK = 512, 64, 576
ROW_GROUP, KEY_STEP, MAX_T, MAX_HQ = 64, 64, 8, 128
LOG2E = cr.LOG2E
NEG_INF = float("-inf")
INT_MAX = 2 ** 31 - 1
SCALE = 192 ** -0.5   # the models' scale without mscale, and the scale of the test data
FILL = 2.0 ** 100     # what the pages no live table entry names hold
YARN = SCALE * (0.1 * math.log(40) + 1) ** 2  # DeepSeek-V3 / R1 with YaRN (mscale^2 at factor 40): about 0.1353
QUARTER = SCALE / 4
OTHER_SCALES = (YARN, QUARTER)  # scales that are not the test data's
# q and the rows are N(0, 1 / 192): q . row has standard deviation 0.125 and the scores, under any of the scales, 0.02 at the most -- a softmax
# too flat to tell one scale from another. q x 2^7 (exact in bf16) is the smallest power of two at which every (3, 5) and (2, 40) case of the
# three decode entries, at both KV_SCALES, meets sees_the_scale() at both OTHER_SCALES; found on the CPU, asserted by the surface tests.
Q_MULT = 128
SENSITIVITY = 20


# ---------------------------------------------------------------------------------------------------- reference and emulation

def gather(pool, block_table, lens):
    """Dense [B, Nmax, dk] from pool [P, page, dk]; only the entries 0 .. ceil(len_b / page) - 1 of a table row are followed."""
    P, page, dk = pool.shape
    B, max_pages = block_table.shape
    out = torch.zeros(B, max_pages * page, dk, dtype=pool.dtype)
    for b in range(B):
        n = min(max(int(lens[b]), 0), max_pages * page)
        for i in range(-(-n // page)):
            out[b, i * page:(i + 1) * page] = pool[int(block_table[b, i])]
    return out


def emul_rows(q, rows, vis, scale, dv):
    """O_emul fp64 [R, dv] holding bf16 values: queries q [R, dk] over latent rows [N, dk] (bf16), query r seeing the first vis[r] keys."""
    R = q.shape[0]
    out = torch.zeros(R, dv, dtype=torch.float64)
    top = int(max(vis)) if len(vis) else 0
    if top == 0:
        return out
    vist = torch.tensor(list(vis), dtype=torch.int64)
    live = vist > 0
    s = (q.double() @ rows[:top].double().T).float() * torch.tensor(cr.f32(scale) * LOG2E, dtype=torch.float32)   # 1
    s = s.masked_fill(torch.arange(top)[None, :] >= vist[:, None], NEG_INF)[live]
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)                                                      # 2
    lsum = p.sum(dim=-1, dtype=torch.float32)                                                                    # 5: of the unrounded P
    o = p.bfloat16().double() @ rows[:top, :dv].double()                                                         # 3, 4
    out[live] = (o / lsum.double()[:, None]).float().bfloat16().double()                                         # 5, 6
    return out


def decode(q, pool, block_table, lens, scale, dv=DC):
    """(O [B,T,Hq,dv], LSE [B,T,Hq], O_emul [B,T,Hq,dv]), all fp64: q bf16 [B,T,Hq,dk], pool bf16 [P,page,dk]."""
    B, T, Hq, dk = q.shape
    Nmax = block_table.shape[1] * pool.shape[1]
    dense = gather(pool, block_table, lens)
    vis = mr.visible(lens, T, Nmax)
    x = cr.f32(scale)
    O = torch.zeros(B, T, Hq, dv, dtype=torch.float64)
    L = torch.full((B, T, Hq), NEG_INF, dtype=torch.float64)
    E = torch.zeros(B, T, Hq, dv, dtype=torch.float64)
    for b in range(B):
        vb = vis[b * T:(b + 1) * T]
        top = max(vb)
        if top == 0:
            continue
        rows = dense[b, :top].double()
        vist = torch.tensor(vb)
        live = vist > 0
        hidden = (torch.arange(top)[None, :] >= vist[:, None])[live]
        for h in range(Hq):
            s = (q[b, live, h].double() @ rows.T * x).masked_fill(hidden, NEG_INF)
            lse = torch.logsumexp(s, dim=-1)
            O[b, live, h] = torch.exp(s - lse[:, None]) @ rows[:, :dv]
            L[b, live, h] = lse
            E[b, :, h] = emul_rows(q[b, :, h], dense[b], vb, scale, dv)
    return O, L, E


# ---------------------------------------------------------------------------------------------------- the plan, restated

def plan_rule(B, T, Hq, max_pages, page):
    """fa2d::split_plan(bk = B ceil(T Hq / 64), rows = B T Hq, Nmax, unit = max(page, 64), D = 512): split until bk S reaches 1024 workgroups
    but into chunks of at least 256 keys and at most 64 splits; chunk a multiple of the unit; workspace rows S (512 + 2) 4 bytes when S > 1."""
    Nmax, U = max_pages * page, max(page, KEY_STEP)
    bk, want = B * (-(-T * Hq // ROW_GROUP)), 1
    if bk < 1024 and Nmax > 256:
        want = min((1024 + bk - 1) // bk, Nmax // 256, 64)
    chunk = ((Nmax + want - 1) // want + U - 1) // U * U
    splits = (Nmax + chunk - 1) // chunk
    return splits, chunk, (B * T * Hq * splits * (DC + 2) * 4 if splits > 1 else 0)


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test

def make_pool(dense, page, lens, seed=0):
    """(pool [P,page,dk], block_table int32 [B,max_pages]) of dense latent rows [B,Nmax,dk], as paged_decode_reference.make_pool builds its
    pools: the live pages interleaved and placed by a seeded permutation, every page no live entry names filled with 2^100, every table entry past
    ceil(len_b / page) pointing at such a page."""
    import paged_decode_reference as pr
    kp, _, bt = pr.make_pool(dense[:, None], dense[:, None, :, :1], page, lens, seed=seed, fill=FILL)
    return kp[:, 0].contiguous(), bt


ONE_LENS = [0, 1, 17, 63, 64, 65, 100, 257]
ONE_LENS_SHORT = [0, 1, 2, 5, 7, 8, 100, 257]  # for T = 8: lengths below T, whose first tokens see no key
ONE_NMAX = 320                                 # a multiple of 16 and 64 above 257
ONE_TH = [(1, 1), (1, 16), (1, 17), (3, 5), (1, 64), (5, 13), (2, 128), (8, 3)]
SPLIT_LENS, SPLIT_PAGE, SPLIT_MAX_PAGES = [1000, 300, 257, 100, 0], 16, 64
SPLIT_TH = [(1, 16), (2, 40), (1, 128)]
COUNT_N = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def _randn(shape, g):
    return (torch.randn(*shape, generator=g) * SCALE).to(BF)


@functools.lru_cache(maxsize=None)
def _dense(B, Nmax):
    return _randn((B, Nmax, DK), torch.Generator().manual_seed(7 * B + Nmax))


@functools.lru_cache(maxsize=None)
def one_case(T, Hq, page):
    """case 1: (q [8,T,Hq,576], lens, (pool, block_table)); one split."""
    lens = ONE_LENS_SHORT if T == 8 else ONE_LENS
    q = _randn((len(lens), T, Hq, DK), torch.Generator().manual_seed(100 * T + Hq + page))
    return q, lens, make_pool(_dense(len(lens), ONE_NMAX), page, lens, seed=T + Hq)


@functools.lru_cache(maxsize=None)
def split_case(T, Hq):
    """case 2: (q [5,T,Hq,576], lens, (pool, block_table)); Nmax 1024 at page 16."""
    q = _randn((len(SPLIT_LENS), T, Hq, DK), torch.Generator().manual_seed(1000 * T + Hq))
    return q, SPLIT_LENS, make_pool(_dense(len(SPLIT_LENS), SPLIT_PAGE * SPLIT_MAX_PAGES), SPLIT_PAGE, SPLIT_LENS, seed=Hq)


# ---------------------------------------------------------------------------------------------------- a scale that is not the data's

def times(q, mult):
    """q x a power of two, exact in bf16."""
    out = (q.float() * mult).to(BF)
    assert torch.equal(out.float(), q.float() * mult)
    return out


def sees_the_scale(ref, ref_at_data_scale):
    """(max |O_ref(scale) - O_ref(SCALE)|, SENSITIVITY x o_bound at scale): a kernel that ran at SCALE whatever it was given is far outside
    the bound iff the first exceeds the second (test_rotary_dims_reach_the_scores' condition)."""
    import paged_bf16_reference as br
    ro, _, emul = ref
    fin = torch.isfinite(ro)
    return float((ro[fin] - ref_at_data_scale[0][fin]).abs().max()), SENSITIVITY * br.o_bound(emul, ro)


SCALE_TH = [(3, 5, False), (2, 40, True)]  # (T, Hq, several splits): one_case at page 16 and split_case


@functools.lru_cache(maxsize=None)
def scale_case(T, Hq, split, scale):
    """(q x Q_MULT, lens, (pool, block_table), the reference at scale, the reference at SCALE) of one_case(T, Hq, 16) or split_case(T, Hq)."""
    q, lens, pool = split_case(T, Hq) if split else one_case(T, Hq, 16)
    q = times(q, Q_MULT)
    return q, lens, pool, decode(q, *pool, lens, scale), decode(q, *pool, lens, SCALE)
