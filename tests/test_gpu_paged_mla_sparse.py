"""GPU: sparse multi-head latent attention over the paged latent cache -- cuda_learn_notes_amd.fa2_decode_paged_mla_sparse_bf16
(csrc/flash_attn_decode_paged_mla_sparse_bf16.*) -- against tests/paged_mla_sparse_reference.py (fp64 and the bf16 emulation,
anchored to paged_mla_reference.decode by tests/test_paged_mla_sparse_surface.py). No new tolerance: O within paged_bf16_reference.o_bound of
the emulation, LSE within decode_reference.lse_tol per head, -inf LSE entries and zero rows exactly (test_gpu_paged_sink_attention.check).
Beyond parity: bit equality with fa2_decode_paged_mla_bf16 on the dense list, exact counts (q = 0, value dims 1: O = 1, LSE = ln of the
valid slots) with a valid slot on each side of every step, chunk and list edge, empty slots of every kind in front of guard entries that
name a page of NaNs, NaN in every unlisted pool row, duplicates, many query tokens, and bit equalities -- a sequence alone, two calls, guard
bands, a captured graph. Every parity case prints err / bound before it asserts (pytest -s); the last test prints the largest per group.

Largest err / bound of O seen on an MI355X: see DESIGN 4.4.20 and profiles/r30_paged_mla_sparse_tests.log."""
import math
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_edge_cases as ec  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DC, DK, SCALE = ml.DC, ml.DK, ml.SCALE
O_FILL, L_FILL = sk.O_FILL, sk.L_FILL
NEG_INF = float("-inf")
bits, fbits, check = sk.bits, sk.fbits, sk.check
RATIOS = {}


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def plan(B, T, Hq, topk, pool):
    return pkg().fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, topk, pool[1].shape[1], pool[0].shape[1])


def sparse(q, pool, lens, idx, scale=SCALE, table=None, dev="cuda"):
    """(o, lse) on the CPU; the workspace is sized from the entry's own plan. table: a block table that is on the device already."""
    c = pkg()
    qd, pd = q.to(dev), pool[0].to(dev)
    bd = pool[1].to(dev) if table is None else table
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    B, T, Hq, _ = q.shape
    o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    ws = torch.empty(max(plan(B, T, Hq, idx.shape[2], pool)[2], 16), dtype=torch.uint8, device=dev)
    c.fa2_decode_paged_mla_sparse_bf16(qd, pd, bd, sl, idx.to(dev), scale, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def dense(q, pool, lens, scale=SCALE, dev="cuda"):
    """(o, lse) of fa2_decode_paged_mla_bf16 on the CPU."""
    c = pkg()
    B, T, Hq, _ = q.shape
    o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    need = c.fa2_decode_paged_mla_bf16_plan(B, T, Hq, pool[1].shape[1], pool[0].shape[1])[2]
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    c.fa2_decode_paged_mla_bf16(q.to(dev), pool[0].to(dev), pool[1].to(dev), torch.tensor(list(lens), dtype=torch.int32, device=dev), scale, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def same(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(fbits(a[1]), fbits(b[1]))


def reference(q, pool, lens, idx):
    return sp.decode_sparse(q, pool[0], pool[1], lens, idx, SCALE)


# ---------------------------------------------------------------------------------------------------- 1. parity, one split

@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("TH", sp.ONE_TH, ids=lambda th: "T%dxHq%d" % th)
def test_parity_one_split(built, dev, TH, page):
    """Lengths 0, 1, 17, 63, 64, 65, 100, 257 (at T = 8: 0, 1, 2, 5, 7, 8, 100, 257) at Nmax 320, topk 1, 63, 64, 65, 200: lists of
    min(vis, about 2/3 topk) distinct visible positions, unsorted, scattered over the slots with empty slots between them; Hq from 1 head to
    two head groups, 17 and 65 leaving one head to a second tile resp. a second group."""
    T, Hq = TH
    q, lens, pool = sp.one_case(T, Hq, page)
    for topk in sp.ONE_TOPK:
        idx = sp.one_indices(T, Hq, page, topk)
        assert plan(len(lens), T, Hq, topk, pool)[0] == 1
        got = sparse(q, pool, lens, idx)
        ro, rl, emul = reference(q, pool, lens, idx)
        assert bool((rl[0] == NEG_INF).all()) and bool(torch.isfinite(rl[-1]).all())
        note("parity, one split", check(*got, ro, rl, emul, "mla sparse S=1 T=%d Hq=%d page=%d topk=%d" % (T, Hq, page, topk)))


# ---------------------------------------------------------------------------------------------------- 2. several splits

@pytest.mark.parametrize("TH", sp.SPLIT_TH, ids=lambda th: "T%dxHq%d" % th)
def test_parity_several_splits(built, dev, TH):
    """topk 2048 and B = 5: 8 splits of 256 slots. Page 16, 256 table entries, lengths 4000, 2048, 300, 100 and 0. The length-100 sequence
    runs twice: its valid slots all in the first chunk, then all in the last one -- seven of its eight splits are empty either way. The
    length-0 sequence: O = 0, LSE = -inf."""
    T, Hq = TH
    q, lens, pool = sp.split_case(T, Hq)
    S, C, _ = plan(len(lens), T, Hq, sp.SPLIT_TOPK, pool)
    assert (S, C) == (8, 256), (S, C)
    for last in (False, True):
        idx = sp.split_indices(T, Hq, last)
        slots = [k for k, _ in sp.valid_slots(idx[3, T - 1], 100)]
        assert len(slots) == 100 and (min(slots) >= 1792 if last else max(slots) < 256)
        got = sparse(q, pool, lens, idx)
        ro, rl, emul = reference(q, pool, lens, idx)
        note("parity, several splits", check(*got, ro, rl, emul, "mla sparse S=%d T=%d Hq=%d len-100 slots %s" % (S, T, Hq, "last" if last else "first")))
        assert bool((bits(got[0][4]) == 0).all()) and bool((got[1][4] == NEG_INF).all())


# ---------------------------------------------------------------------------------------------------- 2b. a scale that is not the data's

@pytest.mark.parametrize("scale", ml.OTHER_SCALES, ids=["yarn", "quarter"])
@pytest.mark.parametrize("case", ml.SCALE_TH, ids=lambda c: "T%dxHq%d%s" % (c[0], c[1], "-split" if c[2] else ""))
def test_parity_at_a_scale_that_is_not_the_datas(built, dev, case, scale):
    """The one-split case at (3, 5), topk 200, and the several-splits case at (2, 40), topk 2048, at V3's YaRN scale and at SCALE / 4,
    q x Q_MULT: the reference at SCALE is more than 20 x o_bound away (proven without a GPU by tests/test_paged_mla_sparse_surface.py)."""
    T, Hq, split = case
    q, lens, pool, idx, ref, ref0 = sp.scale_case(T, Hq, split, scale)
    S = plan(len(lens), T, Hq, idx.shape[2], pool)[0]
    assert (S > 1) == split
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla sparse scale %.5f T=%d Hq=%d S=%d: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, T, Hq, S, diff, need))
    assert diff > need
    note("parity, another scale", check(*sparse(q, pool, lens, idx, scale=scale), *ref, "mla sparse scale=%.5f S=%d T=%d Hq=%d" % (scale, S, T, Hq)))


def _graph_replays_eager(call, B, T, Hq, need):
    """call(o, lse, ws) eager, then captured in a graph and replayed on fresh buffers: (eager o, lse on the CPU), bit for bit the replay's."""
    def buffers():
        return (torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device="cuda").view(BF),
                torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device="cuda").view(torch.float32), torch.empty(need, dtype=torch.uint8, device="cuda"))

    eager = buffers()
    call(*eager)
    torch.cuda.synchronize()
    o, lse = eager[0].cpu(), eager[1].cpu()
    bufs = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(*bufs)
    torch.cuda.synchronize()
    assert bool((bits(bufs[0].cpu()) == O_FILL).all())  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(bufs[0].cpu()), bits(o)) and torch.equal(fbits(bufs[1].cpu()), fbits(lse))
    return o, lse


def test_parity_at_the_yarn_scale_through_a_captured_graph(built, dev):
    """The several-splits case at (2, 40) at YARN: the stream kernel and the combine captured and replayed, bit for bit the eager result."""
    c = pkg()
    T, Hq = 2, 40
    q, lens, pool, idx, ref, _ = sp.scale_case(T, Hq, True, ml.YARN)
    B = len(lens)
    S, _, need = plan(B, T, Hq, idx.shape[2], pool)
    assert S > 1
    fixed = (q.to("cuda"), pool[0].to("cuda"), pool[1].to("cuda"), torch.tensor(lens, dtype=torch.int32, device="cuda"), idx.to("cuda"))
    o, lse = _graph_replays_eager(lambda o, lse, ws: c.fa2_decode_paged_mla_sparse_bf16(*fixed, ml.YARN, o, lse, ws), B, T, Hq, need)
    note("parity, another scale", check(o, lse, *ref, "mla sparse scale=YARN eager, then a captured graph S=%d" % S))


# ---------------------------------------------------------------------------------------------------- 3. bits of the dense entry

@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("TH", sp.ONE_TH, ids=lambda th: "T%dxHq%d" % th)
def test_dense_list_gives_the_bits_of_the_dense_entry_one_split(built, dev, TH, page):
    """indices[b, t] = [0 ... vis - 1] then -1 up to topk = Nmax = 320: O and LSE are fa2_decode_paged_mla_bf16's bit for bit (both plans: one
    split). Pins the step order, the mask and the stores to a kernel that is already trusted."""
    T, Hq = TH
    q, lens, pool = sp.one_case(T, Hq, page)
    idx = sp.dense_indices(lens, T, sp.ONE_NMAX, sp.ONE_NMAX)
    assert plan(len(lens), T, Hq, sp.ONE_NMAX, pool)[0] == 1 and pkg().fa2_decode_paged_mla_bf16_plan(len(lens), T, Hq, pool[1].shape[1], page)[0] == 1
    assert same(sparse(q, pool, lens, idx), dense(q, pool, lens))


@pytest.mark.parametrize("Hq", [16, 128])
def test_dense_list_gives_the_bits_of_the_dense_entry_several_splits(built, dev, Hq):
    """Nmax = topk = 1024, page 16, T = 1, lengths 1000, 300, 257, 100, 0: both plans give 4 splits of 256. The dense combine merges the live
    splits of a row, the new one all four: an empty split changes no bit."""
    q, lens, pool = ml.split_case(1, Hq)
    idx = sp.dense_indices(lens, 1, 1024, 1024)
    assert plan(len(lens), 1, Hq, 1024, pool)[:2] == pkg().fa2_decode_paged_mla_bf16_plan(len(lens), 1, Hq, 64, 16)[:2] == (4, 256)
    assert same(sparse(q, pool, lens, idx), dense(q, pool, lens))


# ---------------------------------------------------------------------------------------------------- 4. exact counts

EDGE_SLOTS = {320: (0, 63, 64, 319), 2048: (0, 63, 64, 255, 256, 2047)}  # 0, 63, 64, C - 1, C, topk - 1


@pytest.mark.parametrize("topk", [320, 2048], ids=["one-split", "several-splits"])
@pytest.mark.parametrize("TH", [(1, 16), (3, 5)], ids=lambda th: "T%dxHq%d" % th)
def test_exact_counts(built, dev, TH, topk):
    """q = 0, value dims = 1, rotary dims random: every weight of a row is 1 / n, so O is exactly 1 and LSE = ln n, n = the valid slots of the
    token: 1 ... 257 of them (paged_mla_reference.COUNT_N, one sequence each, length 300), the first ones on the slots 0, 63, 64, C - 1, C and
    topk - 1 -- one on each side of every step, chunk and list edge -- the others scattered."""
    T, Hq = TH
    counts, page, max_pages = ml.COUNT_N, 16, 20
    B, lens = len(counts), [300] * len(counts)
    g = torch.Generator().manual_seed(topk)
    dense_rows = torch.ones(1, max_pages * page, DK)
    dense_rows[..., DC:] = torch.randn(1, max_pages * page, ml.DR, generator=g)
    pool = ml.make_pool(dense_rows.to(BF).expand(B, -1, -1), page, lens, seed=3)
    S, C, _ = plan(B, T, Hq, topk, pool)
    assert (S, C) == ((1, 320) if topk == 320 else (8, 256)), (S, C)
    rnd = random.Random(topk + T)
    idx = torch.full((B, T, topk), -1, dtype=torch.int32)
    edges = EDGE_SLOTS[topk]
    for b, n in enumerate(counts):
        for t in range(T):
            rest = [k for k in range(topk) if k not in edges]
            slots = (list(edges) + rnd.sample(rest, max(n - len(edges), 0)))[:n]
            for k, p in zip(slots, rnd.sample(range(300 - (T - 1 - t)), n)):
                idx[b, t, k] = p
    q = torch.zeros(B, T, Hq, DK, dtype=BF)
    o, lse = sparse(q, pool, lens, idx)
    worst = 0.0
    for b, n in enumerate(counts):
        for t in range(T):
            assert bool((o[b, t] == 1).all()), (b, t, n)
            err, tol = (lse[b, t].double() - math.log(n)).abs().max().item(), ec.lse_tol_at(n)
            worst = max(worst, err / tol)
            assert err <= tol, (b, t, n, err, tol)
    print("mla sparse counts T=%d Hq=%d S=%d: LSE = ln(valid slots) within %.4f of the tolerance" % (T, Hq, S, worst))


# ---------------------------------------------------------------------------------------------------- 5. empty slots of every kind

def test_empty_slots_of_every_kind(built, dev):
    """A list of case 1 with its empty slots replaced, in turn, by -1, -7, vis itself, len, Nmax - 1 and Nmax + 5 (all below 2 Nmax): bit for
    bit the all-(-1) form. The table is a view into a larger int32 buffer whose guard entries name an allocated page of NaNs, and the table
    entries past a sequence's pages name pages of 2^100: a kernel that followed an empty slot would give a wrong answer, never a stray access."""
    T, Hq, page, topk = 3, 5, 16, 200
    q, lens, (pool, bt) = sp.one_case(T, Hq, page)
    idx = sp.one_indices(T, Hq, page, topk)
    Nmax, (B, max_pages) = sp.ONE_NMAX, bt.shape
    vis = sp.visible(lens, T, Nmax)
    odd = idx.clone()
    n_odd = 0
    for b in range(B):
        for t in range(T):
            kinds = [-1, -7, vis[b][t], lens[b], Nmax - 1, Nmax + 5]
            assert all(not 0 <= k < vis[b][t] and k < 2 * Nmax for k in kinds)
            for k in range(topk):
                if idx[b, t, k] == -1:
                    odd[b, t, k] = kinds[n_odd % 6]
                    n_odd += 1
    assert n_odd > 1000 and not torch.equal(odd, idx)
    assert all(torch.equal(a, b_) for a, b_ in zip(reference(q, (pool, bt), lens, odd), reference(q, (pool, bt), lens, idx)))
    pool_n = torch.cat([pool, torch.full((1, page, DK), float("nan"), dtype=BF)])
    guard = 2 * max_pages
    big = torch.full((B * max_pages + 2 * guard,), pool.shape[0], dtype=torch.int32, device="cuda")
    table = big[guard:guard + B * max_pages].view(B, max_pages)
    table.copy_(bt.to("cuda"))
    base = sparse(q, (pool_n, bt), lens, idx, table=table)
    got = sparse(q, (pool_n, bt), lens, odd, table=table)
    assert bool(torch.isfinite(got[0].float()).all()) and same(got, base)
    note("parity, one split", check(*got, *reference(q, (pool, bt), lens, idx), "mla sparse empty slots of every kind"))
    assert bool((big[:guard] == pool.shape[0]).all()) and bool((big[-guard:] == pool.shape[0]).all())


# ---------------------------------------------------------------------------------------------------- 6. unlisted rows do not matter

@pytest.mark.parametrize("several", [False, True], ids=["one-split", "several-splits"])
def test_unlisted_pool_rows_may_hold_nan(built, dev, several):
    """Every pool row that no valid slot of any token names holds NaN -- whole pages inside the sequences among them: the output is finite and
    bit for bit that of the clean pool."""
    if several:
        T, Hq = 2, 40
        (q, lens, (pool, bt)), idx = sp.split_case(T, Hq), sp.split_indices(T, Hq, True)
    else:
        T, Hq, page, topk = 3, 5, 16, 65
        (q, lens, (pool, bt)), idx = sp.one_case(T, Hq, page), sp.one_indices(T, Hq, page, topk)
    idx = idx.clone()
    idx[(idx >= 32) & (idx < 64)] = -1  # the positions 32 ... 63 of every sequence are listed by no token: two to four whole pages
    page = pool.shape[1]
    vis = sp.visible(lens, T, bt.shape[1] * page)
    named = torch.zeros(pool.shape[:2], dtype=torch.bool)
    for b in range(len(lens)):
        for t in range(T):
            for _, p in sp.valid_slots(idx[b, t], vis[b][t]):
                named[int(bt[b, p // page]), p % page] = True
    dirty = pool.clone()
    dirty[~named] = float("nan")
    live_pages = {int(bt[b, i]) for b, n in enumerate(lens) for i in range(-(-n // page))}
    assert any(not bool(named[p].any()) for p in live_pages) and int(named.sum()) > 100  # whole pages inside a sequence are unlisted
    clean, got = sparse(q, (pool, bt), lens, idx), sparse(q, (dirty, bt), lens, idx)
    assert bool(torch.isfinite(got[0].float()).all()) and not bool(torch.isnan(got[1]).any()) and same(got, clean)


# ---------------------------------------------------------------------------------------------------- 7. duplicates

def test_a_position_listed_twice_is_two_keys(built, dev):
    """Every valid position of a list a second time in an empty slot: the reference counts it twice, and so does the kernel (LSE moves by ln 2
    against the list without duplicates)."""
    T, Hq, page, topk = 3, 5, 16, 200
    q, lens, pool = sp.one_case(T, Hq, page)
    idx = sp.one_indices(T, Hq, page, 64)  # at most 43 valid slots of 64
    dup = torch.full((len(lens), T, topk), -1, dtype=torch.int32)
    dup[:, :, :64] = idx
    dup[:, :, 100:164] = idx
    got = sparse(q, pool, lens, dup)
    ro, rl, emul = reference(q, pool, lens, dup)
    once = reference(q, pool, lens, idx)[1]
    fin = torch.isfinite(rl)
    assert float((rl[fin] - once[fin] - math.log(2)).abs().max()) < 1e-9
    note("duplicates", check(*got, ro, rl, emul, "mla sparse duplicates T=%d Hq=%d" % (T, Hq)))


# ---------------------------------------------------------------------------------------------------- 8. many tokens

@pytest.mark.parametrize("TH", sp.MANY_TH, ids=lambda th: "T%dxHq%d" % th)
def test_many_query_tokens(built, dev, TH):
    """T = 33 and 70, past the dense entry's cap of 8, at lengths 100 and 20, topk 64: the causal edge moves per token, the first tokens of the
    length-100 sequence see fewer keys than the last (at T = 70 fewer than the list could hold: 31) and those of the length-20 one none."""
    T, Hq = TH
    q, lens, pool, idx = sp.many_case(T, Hq)
    got = sparse(q, pool, lens, idx)
    ro, rl, emul = reference(q, pool, lens, idx)
    assert bool((rl[1, 0] == NEG_INF).all()) and bool(torch.isfinite(rl[0]).all()) and bool(torch.isfinite(rl[1, T - 1]).all())
    assert len(sp.valid_slots(idx[0, 0], 100 - (T - 1))) == min(100 - (T - 1), 43) and len(sp.valid_slots(idx[0, T - 1], 100)) == 43
    assert 100 - (T - 1) < sp.MANY_TOPK or T == 33
    note("many tokens", check(*got, ro, rl, emul, "mla sparse T=%d Hq=%d" % (T, Hq)))


# ---------------------------------------------------------------------------------------------------- 9. independence and guard bands

def test_a_sequence_alone_two_calls_and_guard_bands(built, dev):
    c = pkg()
    T, Hq, page, topk = 1, 16, 16, 200
    q, lens, (pool, bt) = sp.one_case(T, Hq, page)
    idx = sp.one_indices(T, Hq, page, topk)
    B = len(lens)
    base = sparse(q, (pool, bt), lens, idx)
    assert same(sparse(q, (pool, bt), lens, idx), base)  # two calls
    for b in range(B):  # alone: B = 1 with its table row and its list (the plan is one split for either B)
        one = sparse(q[b:b + 1].contiguous(), (pool, bt[b:b + 1].contiguous()), lens[b:b + 1], idx[b:b + 1].contiguous())
        assert same(one, (base[0][b:b + 1], base[1][b:b + 1])), b
    # guard bands around o and lse, one split
    dv = "cuda"
    big_o = torch.full((B + 2, T, Hq, DC), O_FILL, dtype=torch.int16, device=dv).view(BF)
    big_l = torch.full((B + 2, T, Hq), L_FILL, dtype=torch.int32, device=dv).view(torch.float32)
    sl = torch.tensor(lens, dtype=torch.int32, device=dv)
    c.fa2_decode_paged_mla_sparse_bf16(q.to(dv), pool.to(dv), bt.to(dv), sl, idx.to(dv), SCALE, big_o[1:B + 1], big_l[1:B + 1])
    torch.cuda.synchronize()
    assert same((big_o[1:B + 1].cpu(), big_l[1:B + 1].cpu()), base)
    for edge in (0, B + 1):
        assert bool((bits(big_o[edge].cpu()) == O_FILL).all()) and bool((fbits(big_l[edge].cpu()) == L_FILL).all())
    # several splits: two calls, a sequence alone (8 splits for either B), guard bands around o, lse and the workspace, lse = None
    T, Hq = 2, 40
    q, lens, (pool, bt) = sp.split_case(T, Hq)
    idx = sp.split_indices(T, Hq, False)
    B = len(lens)
    base = sparse(q, (pool, bt), lens, idx)
    assert same(sparse(q, (pool, bt), lens, idx), base)
    for b in (0, 3):
        assert plan(1, T, Hq, sp.SPLIT_TOPK, (pool, bt))[:2] == (8, 256)
        one = sparse(q[b:b + 1].contiguous(), (pool, bt[b:b + 1].contiguous()), lens[b:b + 1], idx[b:b + 1].contiguous())
        assert same(one, (base[0][b:b + 1], base[1][b:b + 1])), b
    need = plan(B, T, Hq, sp.SPLIT_TOPK, (pool, bt))[2]
    band = 4096
    big_o = torch.full((B + 2, T, Hq, DC), O_FILL, dtype=torch.int16, device=dv).view(BF)
    big_l = torch.full((B + 2, T, Hq), L_FILL, dtype=torch.int32, device=dv).view(torch.float32)
    big_w = torch.full((need + 2 * band,), 0x5A, dtype=torch.uint8, device=dv)
    args = (q.to(dv), pool.to(dv), bt.to(dv), torch.tensor(lens, dtype=torch.int32, device=dv), idx.to(dv), SCALE)
    c.fa2_decode_paged_mla_sparse_bf16(*args, big_o[1:B + 1], big_l[1:B + 1], big_w[band:band + need])
    torch.cuda.synchronize()
    assert same((big_o[1:B + 1].cpu(), big_l[1:B + 1].cpu()), base)
    for edge in (0, B + 1):
        assert bool((bits(big_o[edge].cpu()) == O_FILL).all()) and bool((fbits(big_l[edge].cpu()) == L_FILL).all())
    assert bool((big_w[:band] == 0x5A).all()) and bool((big_w[band + need:] == 0x5A).all()) and not bool((big_w[band:band + need] == 0x5A).all())
    o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=dv).view(BF)
    c.fa2_decode_paged_mla_sparse_bf16(*args, o)  # lse = None, the workspace allocated by the entry
    torch.cuda.synchronize()
    assert torch.equal(bits(o.cpu()), bits(base[0]))


# ---------------------------------------------------------------------------------------------------- 10. captured graph

def test_captured_graph_replays_the_eager_bits(built, dev):
    """The several-splits call (stream kernel + combine) captured in a graph and replayed on fresh buffers: bit for bit the eager result."""
    c = pkg()
    T, Hq = 2, 40
    q, lens, (pool, bt) = sp.split_case(T, Hq)
    idx = sp.split_indices(T, Hq, True)
    B = len(lens)
    S, _, need = plan(B, T, Hq, sp.SPLIT_TOPK, (pool, bt))
    assert S > 1
    dv = "cuda"
    fixed = (q.to(dv), pool.to(dv), bt.to(dv), torch.tensor(lens, dtype=torch.int32, device=dv), idx.to(dv))

    def buffers():
        return (torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=dv).view(BF),
                torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=dv).view(torch.float32), torch.empty(need, dtype=torch.uint8, device=dv))

    def step(o, lse, ws):
        c.fa2_decode_paged_mla_sparse_bf16(*fixed, SCALE, o, lse, ws)

    eager = buffers()
    step(*eager)
    torch.cuda.synchronize()
    o, lse = eager[0].cpu(), eager[1].cpu()
    note("captured graph", check(o, lse, *reference(q, (pool, bt), lens, idx), "mla sparse eager, then a captured graph T=%d Hq=%d S=%d" % (T, Hq, S)))
    graph_bufs = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(*graph_bufs)
    torch.cuda.synchronize()
    assert bool((bits(graph_bufs[0].cpu()) == O_FILL).all())  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(graph_bufs[0].cpu()), bits(o)) and torch.equal(fbits(graph_bufs[1].cpu()), fbits(lse))


# ---------------------------------------------------------------------------------------------------- 11. summary

def test_zz_summary_of_error_over_bound(built, dev):
    """The RATIOS table: the largest O err / bound of every group of parity cases of this file. Not an assertion of its own --
    every case asserted err <= bound where it ran."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
