"""GPU: sparse multi-head latent attention over a paged latent cache held in FP8 -- cuda_learn_notes_amd.fa2_decode_paged_mla_sparse_bf16_fp8
(csrc/flash_attn_decode_paged_mla_sparse_bf16_fp8.*) -- against tests/paged_mla_sparse_fp8_reference.py (fp64 on the dequantised
rows and the bf16 emulation on the codes, anchored to the two siblings' references by tests/test_paged_mla_sparse_fp8_surface.py). No new
tolerance: O within paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol per head, -inf LSE entries and zero
rows exactly (test_gpu_paged_sink_attention.check). Beyond parity: the bits of fa2_decode_paged_mla_bf16_fp8 on the dense list and of
fa2_decode_paged_mla_sparse_bf16 on the dequantised pool at a power-of-two scale, exact counts with a valid slot on each side of every
step, chunk and list edge, empty slots of every kind in front of guard entries that name a page of NaN bytes, NaN bytes in every unlisted pool
row, duplicates, many query tokens, a sequence alone, two calls, guard bands, captured graphs, and the chain of a V3.2 step on FP8 caches.
Every parity case prints err / bound before it asserts (pytest -s); the last test prints the largest per group.

Largest err / bound of O seen on an MI355X: see DESIGN 4.4.23."""
import math
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import paged_edge_cases as ec  # noqa: E402
import paged_mla_fp8_reference as mf  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import paged_mla_sparse_fp8_reference as s8  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F8 = torch.bfloat16, f8.F8
DC, DR, DK, SCALE = ml.DC, ml.DR, ml.DK, ml.SCALE
O_FILL, L_FILL, Q_FILL = sk.O_FILL, sk.L_FILL, 0x3C5A
NEG_INF = float("-inf")
P2 = 2.0 ** -8
NAN_BYTE = s8.NAN_BYTE
bits, fbits, check, cbits = sk.bits, sk.fbits, sk.check, f8.bits
KV_IDS = ["kv2^-8", "kv0.003"]
RATIOS = {}
DEV = "cuda"


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def plan(B, T, Hq, topk, pool):
    return pkg().fa2_decode_paged_mla_sparse_bf16_fp8_plan(B, T, Hq, topk, pool[1].shape[1], pool[0].shape[1])


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def outputs(B, T, Hq):
    return (torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=DEV).view(BF),
            torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=DEV).view(torch.float32))


def sparse(q, pool, lens, idx, kvs, scale=SCALE, table=None):
    """(o, lse) of the new entry on the CPU; the workspace is sized from the entry's own plan. table: a block table already on the device."""
    B, T, Hq, _ = q.shape
    o, lse = outputs(B, T, Hq)
    ws = torch.empty(max(plan(B, T, Hq, idx.shape[2], pool)[2], 16), dtype=torch.uint8, device=DEV)
    pkg().fa2_decode_paged_mla_sparse_bf16_fp8(q.to(DEV), pool[0].to(DEV), pool[1].to(DEV) if table is None else table, i32(lens),
                                               mf.scale_t(kvs).to(DEV), idx.to(DEV), scale, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def sparse_bf16(q, pool, lens, idx, scale=SCALE):
    """(o, lse) of fa2_decode_paged_mla_sparse_bf16 on a bf16 pool."""
    c = pkg()
    B, T, Hq, _ = q.shape
    o, lse = outputs(B, T, Hq)
    need = c.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, idx.shape[2], pool[1].shape[1], pool[0].shape[1])[2]
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    c.fa2_decode_paged_mla_sparse_bf16(q.to(DEV), pool[0].to(DEV), pool[1].to(DEV), i32(lens), idx.to(DEV), scale, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def dense_fp8(q, pool, lens, kvs, scale=SCALE):
    """(o, lse) of fa2_decode_paged_mla_bf16_fp8."""
    c = pkg()
    B, T, Hq, _ = q.shape
    o, lse = outputs(B, T, Hq)
    need = c.fa2_decode_paged_mla_bf16_fp8_plan(B, T, Hq, pool[1].shape[1], pool[0].shape[1])[2]
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    c.fa2_decode_paged_mla_bf16_fp8(q.to(DEV), pool[0].to(DEV), pool[1].to(DEV), i32(lens), mf.scale_t(kvs).to(DEV), scale, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def same(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(fbits(a[1]), fbits(b[1]))


def reference(q, pool, lens, idx, kvs, scale=SCALE):
    return s8.decode_sparse(q, pool[0], pool[1], lens, idx, kvs, scale)


# ---------------------------------------------------------------------------------------------------- 1. parity, one split

@pytest.mark.parametrize("kvs", s8.KV_SCALES, ids=KV_IDS)
@pytest.mark.parametrize("page", s8.ONE_PAGES)
@pytest.mark.parametrize("TH", s8.ONE_TH, ids=lambda th: "T%dxHq%d" % th)
def test_parity_one_split(built, dev, TH, page, kvs):
    """paged_mla_sparse_reference's case 1 quantised on the CPU: lengths 0 ... 257 at Nmax 320, topk 1, 63, 64, 65, 200, lists of distinct
    visible positions scattered over the slots with empty slots between them, Hq from 1 head to two head groups; q x Q_MULT_ONE."""
    T, Hq = TH
    q, lens, pool = s8.one_case(T, Hq, page, kvs)
    for topk in s8.ONE_TOPK:
        idx = s8.one_indices(T, Hq, page, topk)
        assert plan(len(lens), T, Hq, topk, pool)[0] == 1
        got = sparse(q, pool, lens, idx, kvs)
        ro, rl, emul = reference(q, pool, lens, idx, kvs)
        assert bool((rl[0] == NEG_INF).all()) and bool(torch.isfinite(rl[-1]).all())
        note("parity, one split", check(*got, ro, rl, emul, "mla sparse fp8 S=1 T=%d Hq=%d page=%d topk=%d kv_scale=%g" % (T, Hq, page, topk, kvs)))


# ---------------------------------------------------------------------------------------------------- 2. several splits

@pytest.mark.parametrize("kvs", s8.KV_SCALES, ids=KV_IDS)
@pytest.mark.parametrize("TH", s8.SPLIT_TH, ids=lambda th: "T%dxHq%d" % th)
def test_parity_several_splits(built, dev, TH, kvs):
    """topk 2048 and B = 5: 8 splits of 256 slots, lengths 4000, 2048, 300, 100 and 0. The length-100 sequence has its valid slots all in the
    first chunk, then all in the last one: seven of its eight splits are wholly empty; the last split of the length-300 one partly."""
    T, Hq = TH
    q, lens, pool = s8.split_case(T, Hq, kvs)
    S, C, _ = plan(len(lens), T, Hq, sp.SPLIT_TOPK, pool)
    assert (S, C) == (8, 256), (S, C)
    for last in (False, True):
        idx = s8.split_indices(T, Hq, last)
        slots = [k for k, _ in sp.valid_slots(idx[3, T - 1], 100)]
        assert len(slots) == 100 and (min(slots) >= 1792 if last else max(slots) < 256)
        got = sparse(q, pool, lens, idx, kvs)
        ro, rl, emul = reference(q, pool, lens, idx, kvs)
        note("parity, several splits", check(*got, ro, rl, emul, "mla sparse fp8 S=%d T=%d Hq=%d kv_scale=%g len-100 slots %s"
                                             % (S, T, Hq, kvs, "last" if last else "first")))
        assert bool((bits(got[0][4]) == 0).all()) and bool((got[1][4] == NEG_INF).all())


# ---------------------------------------------------------------------------------------------------- 3. another softmax scale, a graph

def _graph_replays_eager(call, B, T, Hq, need):
    """call(o, lse, ws) eager, then captured in a graph and replayed on fresh buffers: (eager o, lse on the CPU), bit for bit the replay's."""
    def buffers():
        return (*outputs(B, T, Hq), torch.empty(max(need, 16), dtype=torch.uint8, device=DEV))

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


@pytest.mark.parametrize("scale", ml.OTHER_SCALES, ids=["yarn", "quarter"])
def test_parity_at_a_scale_that_is_not_the_datas(built, dev, scale):
    """The several-splits case at (2, 40), kv_scale 0.003, at V3's YaRN scale and at SCALE / 4, q x Q_MULT in all: the reference at SCALE is more
    than 20 x o_bound away (proven without a GPU by the surface test), so a constant in the place of softmax_scale would show."""
    T, Hq, kvs = 2, 40, 0.003
    q, lens, pool, idx = s8.scale_case(kvs)
    assert plan(len(lens), T, Hq, sp.SPLIT_TOPK, pool)[0] > 1
    ref, ref0 = reference(q, pool, lens, idx, kvs, scale), reference(q, pool, lens, idx, kvs)
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla sparse fp8 scale %.5f: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, diff, need))
    assert diff > need
    note("parity, another scale", check(*sparse(q, pool, lens, idx, kvs, scale=scale), *ref, "mla sparse fp8 scale=%.5f T=%d Hq=%d" % (scale, T, Hq)))


def test_parity_at_the_yarn_scale_through_a_captured_graph(built, dev):
    """The same case at YARN: the stream kernel and the combine captured and replayed, bit for bit the eager result."""
    c = pkg()
    T, Hq, kvs = 2, 40, 0.003
    q, lens, pool, idx = s8.scale_case(kvs)
    B = len(lens)
    S, _, need = plan(B, T, Hq, sp.SPLIT_TOPK, pool)
    assert S > 1
    fixed = (q.to(DEV), pool[0].to(DEV), pool[1].to(DEV), i32(lens), mf.scale_t(kvs).to(DEV), idx.to(DEV))
    o, lse = _graph_replays_eager(lambda o, lse, ws: c.fa2_decode_paged_mla_sparse_bf16_fp8(*fixed, ml.YARN, o, lse, ws), B, T, Hq, need)
    note("parity, another scale", check(o, lse, *reference(q, pool, lens, idx, kvs, ml.YARN), "mla sparse fp8 YARN eager, then a captured graph S=%d" % S))


# ---------------------------------------------------------------------------------------------------- 4. bits of the siblings

@pytest.mark.parametrize("kvs", s8.KV_SCALES, ids=KV_IDS)
@pytest.mark.parametrize("page", s8.ONE_PAGES)
@pytest.mark.parametrize("TH", [th for th in s8.ONE_TH if th[0] <= 8], ids=lambda th: "T%dxHq%d" % th)
def test_dense_list_gives_the_bits_of_the_dense_fp8_entry_one_split(built, dev, TH, page, kvs):
    """indices[b, t] = [0 ... vis - 1] then -1 up to topk = Nmax = 320: O and LSE are fa2_decode_paged_mla_bf16_fp8's bit for bit (both plans:
    one split). Pins the conversion, the step order, the mask, the two places of kv_scale and the stores to a kernel already trusted."""
    T, Hq = TH
    q, lens, pool = s8.one_case(T, Hq, page, kvs)
    idx = sp.dense_indices(lens, T, sp.ONE_NMAX, sp.ONE_NMAX)
    assert plan(len(lens), T, Hq, sp.ONE_NMAX, pool)[0] == 1 and pkg().fa2_decode_paged_mla_bf16_fp8_plan(len(lens), T, Hq, pool[1].shape[1], page)[0] == 1
    assert same(sparse(q, pool, lens, idx, kvs), dense_fp8(q, pool, lens, kvs))


@pytest.mark.parametrize("kvs", s8.KV_SCALES, ids=KV_IDS)
def test_dense_list_gives_the_bits_of_the_dense_fp8_entry_several_splits(built, dev, kvs):
    """Nmax = topk = 1024, page 16, T = 1, Hq 16, lengths 1000, 300, 257, 100, 0: both plans give 4 splits of 256. The dense combine merges the
    live splits of a row, this one all four: an empty split changes no bit."""
    Hq = 16
    q, lens, pool = mf.split_case(1, Hq, kvs)
    idx = sp.dense_indices(lens, 1, 1024, 1024)
    assert plan(len(lens), 1, Hq, 1024, pool)[:2] == pkg().fa2_decode_paged_mla_bf16_fp8_plan(len(lens), 1, Hq, 64, 16)[:2] == (4, 256)
    assert same(sparse(q, pool, lens, idx, kvs), dense_fp8(q, pool, lens, kvs))


@pytest.mark.parametrize("several", [False, True], ids=["one-split", "several-splits"])
def test_bits_of_the_bf16_sparse_entry_at_a_power_of_two_scale(built, dev, several):
    """kv_scale 2^-8: every product with it is exact, so O and LSE equal fa2_decode_paged_mla_sparse_bf16's on the pool dequantised to bf16 (the
    dead pages zero) bit for bit, on random lists."""
    if several:
        T, Hq = 2, 40
        (q, lens, (pool, bt)), idx = s8.split_case(T, Hq, P2), s8.split_indices(T, Hq, False)
        assert plan(len(lens), T, Hq, idx.shape[2], (pool, bt))[0] == 8
        assert same(sparse(q, (pool, bt), lens, idx, P2), sparse_bf16(q, (s8.deq_bf16(pool, bt, lens, P2), bt), lens, idx))
        return
    for (T, Hq), page, topk in (((3, 5), 16, 200), ((1, 65), 64, 65), ((2, 128), 16, 63)):
        (q, lens, (pool, bt)), idx = s8.one_case(T, Hq, page, P2), s8.one_indices(T, Hq, page, topk)
        assert same(sparse(q, (pool, bt), lens, idx, P2), sparse_bf16(q, (s8.deq_bf16(pool, bt, lens, P2), bt), lens, idx)), (T, Hq, page, topk)


# ---------------------------------------------------------------------------------------------------- 5. exact counts

EDGE_SLOTS = {320: (0, 63, 64, 319), 2048: (0, 63, 64, 255, 256, 2047)}  # 0, 63, 64, C - 1, C, topk - 1


@pytest.mark.parametrize("topk", [320, 2048], ids=["one-split", "several-splits"])
@pytest.mark.parametrize("TH", [(1, 16), (3, 5)], ids=lambda th: "T%dxHq%d" % th)
def test_exact_counts(built, dev, TH, topk):
    """q = 0 (zero scores) and every value code 0x38 = 1.0 at kv_scale 2^-8: every weight of a row is 1 / n, so O is exactly 2^-8 -- O / kv_scale
    times l counts the keys -- and LSE = ln n, n = the valid slots of the token: 1 ... 257 of them (paged_mla_reference.COUNT_N, one sequence
    each, length 300), the first ones on the slots 0, 63, 64, C - 1, C and topk - 1, the others scattered. The rotary codes are random."""
    T, Hq = TH
    counts, page, max_pages = ml.COUNT_N, 16, 20
    B, lens = len(counts), [300] * len(counts)
    g = torch.Generator().manual_seed(topk)
    rows = torch.full((1, max_pages * page, DK), 0x38, dtype=torch.uint8)
    assert float(rows[0, 0, :1].view(F8).float()) == 1.0
    rows[..., DC:] = f8.bits(mf.quantize(torch.randn(1, max_pages * page, DR, generator=g).to(BF), 1.0))
    pool = mf.make_pool(rows.view(F8).expand(B, -1, -1), page, lens, seed=3)
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
    o, lse = sparse(torch.zeros(B, T, Hq, DK, dtype=BF), pool, lens, idx, P2)
    worst = 0.0
    for b, n in enumerate(counts):
        for t in range(T):
            assert bool((o[b, t] == P2).all()), (b, t, n)
            err, tol = (lse[b, t].double() - math.log(n)).abs().max().item(), ec.lse_tol_at(n)
            worst = max(worst, err / tol)
            assert err <= tol, (b, t, n, err, tol)
    print("mla sparse fp8 counts T=%d Hq=%d S=%d: LSE = ln(valid slots) within %.4f of the tolerance" % (T, Hq, S, worst))


# ---------------------------------------------------------------------------------------------------- 6. empty slots, unlisted rows

def test_empty_slots_of_every_kind_and_nan_bytes_in_every_unlisted_row(built, dev):
    """A list of case 1 with its empty slots replaced, in turn, by -1, -7, vis itself, len, Nmax - 1 and Nmax + 5: bit for bit the all-(-1)
    form. The table is a view into a larger int32 buffer whose guard entries name an allocated page of NaN bytes, the table entries past a
    sequence's pages name pages of NaN bytes (make_pool), and every pool row that no valid slot of any token names holds NaN bytes too: a
    kernel that followed an empty slot or read an unlisted row would give NaN, never a stray access."""
    T, Hq, page, topk, kvs = 3, 5, 16, 200, 0.003
    q, lens, (pool, bt) = s8.one_case(T, Hq, page, kvs)
    idx = s8.one_indices(T, Hq, page, topk)
    Nmax, (B, max_pages) = sp.ONE_NMAX, bt.shape
    vis = sp.visible(lens, T, Nmax)
    odd = idx.clone()
    n_odd = 0
    named = torch.zeros(pool.shape[0] + 1, page, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            kinds = [-1, -7, vis[b][t], lens[b], Nmax - 1, Nmax + 5]
            assert all(not 0 <= k < vis[b][t] and k < 2 * Nmax for k in kinds)
            for k in range(topk):
                if idx[b, t, k] == -1:
                    odd[b, t, k] = kinds[n_odd % 6]
                    n_odd += 1
            for _, p in sp.valid_slots(idx[b, t], vis[b][t]):
                named[int(bt[b, p // page]), p % page] = True
    assert n_odd > 1000 and not torch.equal(odd, idx)
    ref = reference(q, (pool, bt), lens, idx, kvs)
    assert all(torch.equal(a, b_) for a, b_ in zip(reference(q, (pool, bt), lens, odd, kvs), ref))
    dirty = torch.cat([cbits(pool), torch.full((1, page, DK), NAN_BYTE, dtype=torch.uint8)])
    dirty[~named] = NAN_BYTE
    assert int(named.sum()) > 100 and int((~named[:-1]).sum()) > 100
    dirty = dirty.view(F8)
    guard = 2 * max_pages
    big = torch.full((B * max_pages + 2 * guard,), pool.shape[0], dtype=torch.int32, device=DEV)
    table = big[guard:guard + B * max_pages].view(B, max_pages)
    table.copy_(bt.to(DEV))
    base = sparse(q, (pool, bt), lens, idx, kvs)
    for lists in (idx, odd):
        got = sparse(q, (dirty, bt), lens, lists, kvs, table=table)
        assert bool(torch.isfinite(got[0].float()).all()) and not bool(torch.isnan(got[1]).any()) and same(got, base)
    note("parity, one split", check(*got, *ref, "mla sparse fp8 empty slots of every kind, NaN bytes in every unlisted row"))
    assert bool((big[:guard] == pool.shape[0]).all()) and bool((big[-guard:] == pool.shape[0]).all())


def test_unlisted_pool_rows_may_hold_nan_bytes_several_splits(built, dev):
    """The several-splits case with the positions 32 ... 63 of every sequence listed by no token: every unlisted row -- whole pages inside the
    sequences among them -- holds NaN bytes; the output is finite and bit for bit that of the clean pool."""
    T, Hq, kvs = 2, 40, P2
    (q, lens, (pool, bt)), idx = s8.split_case(T, Hq, kvs), s8.split_indices(T, Hq, True).clone()
    idx[(idx >= 32) & (idx < 64)] = -1
    page = pool.shape[1]
    vis = sp.visible(lens, T, bt.shape[1] * page)
    named = torch.zeros(pool.shape[:2], dtype=torch.bool)
    for b in range(len(lens)):
        for t in range(T):
            for _, p in sp.valid_slots(idx[b, t], vis[b][t]):
                named[int(bt[b, p // page]), p % page] = True
    dirty = cbits(pool).clone()
    dirty[~named] = NAN_BYTE
    live_pages = {int(bt[b, i]) for b, n in enumerate(lens) for i in range(-(-n // page))}
    assert any(not bool(named[p].any()) for p in live_pages) and int(named.sum()) > 100
    clean, got = sparse(q, (pool, bt), lens, idx, kvs), sparse(q, (dirty.view(F8), bt), lens, idx, kvs)
    assert bool(torch.isfinite(got[0].float()).all()) and not bool(torch.isnan(got[1]).any()) and same(got, clean)


# ---------------------------------------------------------------------------------------------------- 7. duplicates, many tokens

def test_a_position_listed_twice_is_two_keys(built, dev):
    """Every valid position of a list a second time in an empty slot: the reference counts it twice, and so does the kernel (LSE moves by ln 2
    against the list without duplicates)."""
    T, Hq, page, topk, kvs = 3, 5, 16, 200, 0.003
    q, lens, pool = s8.one_case(T, Hq, page, kvs)
    idx = s8.one_indices(T, Hq, page, 64)  # at most 43 valid slots of 64
    dup = torch.full((len(lens), T, topk), -1, dtype=torch.int32)
    dup[:, :, :64] = idx
    dup[:, :, 100:164] = idx
    got = sparse(q, pool, lens, dup, kvs)
    ro, rl, emul = reference(q, pool, lens, dup, kvs)
    once = reference(q, pool, lens, idx, kvs)[1]
    fin = torch.isfinite(rl)
    assert float((rl[fin] - once[fin] - math.log(2)).abs().max()) < 1e-9
    note("duplicates", check(*got, ro, rl, emul, "mla sparse fp8 duplicates T=%d Hq=%d" % (T, Hq)))


@pytest.mark.parametrize("TH", sp.MANY_TH, ids=lambda th: "T%dxHq%d" % th)
def test_many_query_tokens(built, dev, TH):
    """T = 33 and 70, past the dense entry's cap of 8, at lengths 100 and 20, topk 64: the causal edge moves per token, the first tokens of the
    length-100 sequence see fewer keys than the last and those of the length-20 one none."""
    T, Hq = TH
    kvs = 0.003
    q, lens, pool, idx = s8.many_case(T, Hq, kvs)
    got = sparse(q, pool, lens, idx, kvs)
    ro, rl, emul = reference(q, pool, lens, idx, kvs)
    assert bool((rl[1, 0] == NEG_INF).all()) and bool(torch.isfinite(rl[0]).all()) and bool(torch.isfinite(rl[1, T - 1]).all())
    note("many tokens", check(*got, ro, rl, emul, "mla sparse fp8 T=%d Hq=%d" % (T, Hq)))


# ---------------------------------------------------------------------------------------------------- 8. independence and guard bands

def test_a_sequence_alone_two_calls_and_guard_bands(built, dev):
    c = pkg()
    kvs = 0.003
    sc = mf.scale_t(kvs).to(DEV)
    T, Hq, page, topk = 1, 16, 16, 200
    q, lens, (pool, bt) = s8.one_case(T, Hq, page, kvs)
    idx = s8.one_indices(T, Hq, page, topk)
    B = len(lens)
    base = sparse(q, (pool, bt), lens, idx, kvs)
    assert same(sparse(q, (pool, bt), lens, idx, kvs), base)  # two calls
    for b in range(B):  # alone: B = 1 with its table row and its list (the plan is one split for either B)
        one = sparse(q[b:b + 1].contiguous(), (pool, bt[b:b + 1].contiguous()), lens[b:b + 1], idx[b:b + 1].contiguous(), kvs)
        assert same(one, (base[0][b:b + 1], base[1][b:b + 1])), b
    big_o, big_l = outputs(B + 2, T, Hq)  # guard bands around o and lse, one split, the workspace absent
    c.fa2_decode_paged_mla_sparse_bf16_fp8(q.to(DEV), pool.to(DEV), bt.to(DEV), i32(lens), sc, idx.to(DEV), SCALE, big_o[1:B + 1], big_l[1:B + 1])
    torch.cuda.synchronize()
    assert same((big_o[1:B + 1].cpu(), big_l[1:B + 1].cpu()), base)
    for edge in (0, B + 1):
        assert bool((bits(big_o[edge].cpu()) == O_FILL).all()) and bool((fbits(big_l[edge].cpu()) == L_FILL).all())
    # several splits: two calls, a sequence alone (8 splits for either B), guard bands around o, lse and the workspace, lse = None
    T, Hq = 2, 40
    q, lens, (pool, bt) = s8.split_case(T, Hq, kvs)
    idx = s8.split_indices(T, Hq, False)
    B = len(lens)
    base = sparse(q, (pool, bt), lens, idx, kvs)
    assert same(sparse(q, (pool, bt), lens, idx, kvs), base)
    for b in (0, 3):
        assert plan(1, T, Hq, sp.SPLIT_TOPK, (pool, bt))[:2] == (8, 256)
        one = sparse(q[b:b + 1].contiguous(), (pool, bt[b:b + 1].contiguous()), lens[b:b + 1], idx[b:b + 1].contiguous(), kvs)
        assert same(one, (base[0][b:b + 1], base[1][b:b + 1])), b
    need = plan(B, T, Hq, sp.SPLIT_TOPK, (pool, bt))[2]
    band = 4096
    big_o, big_l = outputs(B + 2, T, Hq)
    big_w = torch.full((need + 2 * band,), 0x5A, dtype=torch.uint8, device=DEV)
    args = (q.to(DEV), pool.to(DEV), bt.to(DEV), i32(lens), sc, idx.to(DEV), SCALE)
    c.fa2_decode_paged_mla_sparse_bf16_fp8(*args, big_o[1:B + 1], big_l[1:B + 1], big_w[band:band + need])
    torch.cuda.synchronize()
    assert same((big_o[1:B + 1].cpu(), big_l[1:B + 1].cpu()), base)
    for edge in (0, B + 1):
        assert bool((bits(big_o[edge].cpu()) == O_FILL).all()) and bool((fbits(big_l[edge].cpu()) == L_FILL).all())
    assert bool((big_w[:band] == 0x5A).all()) and bool((big_w[band + need:] == 0x5A).all()) and not bool((big_w[band:band + need] == 0x5A).all())
    o = outputs(B, T, Hq)[0]
    c.fa2_decode_paged_mla_sparse_bf16_fp8(*args, o)  # lse = None, the workspace allocated by the entry
    torch.cuda.synchronize()
    assert torch.equal(bits(o.cpu()), bits(base[0]))


# ---------------------------------------------------------------------------------------------------- 9. the chain of a V3.2 step

def test_chain_of_a_v32_step_on_fp8_caches_eager_and_captured(built, dev):
    """Prompts of [130, 7] tokens in an empty FP8 latent pool and an empty index-key pool; then one step: latent append (interleaved rotation,
    quantising) -> index-key append -> logits -> top-k 64 -> the new entry, Hq 16, eager and replayed from ONE captured graph on fresh state.
    The result is held against the reference on the codes the append wrote and the list the top-k wrote; the graph gives the eager bits."""
    c = pkg()
    kvs, Hq, Hi, page, max_pages, B, topk, P = 0.003, 16, 4, 16, 16, 2, 64, 40
    g = torch.Generator().manual_seed(19)
    prompt = [130, 7]
    lens = [n + 1 for n in prompt]
    ld = max_pages * page
    table = c.kv_append_rope_table(ld, DR).to(DEV)
    bt = torch.randperm(P, generator=g).to(torch.int32)[:B * max_pages].reshape(B, max_pages).contiguous()
    rnd = lambda *s: (torch.randn(*s, generator=g) * SCALE).to(BF)  # noqa: E731
    c0, k0, x0 = rnd(sum(prompt), DC), rnd(sum(prompt), DR), torch.randn(sum(prompt), 128, generator=g).to(BF)
    c1, k1, x1, q1 = rnd(B, DC), rnd(B, DR), torch.randn(B, 128, generator=g).to(BF), ml.times(rnd(B, Hq, DK), 128)
    qi, wt = torch.randn(B, 1, Hi, 128, generator=g).to(BF), torch.rand(B, 1, Hi, generator=g)
    sc = mf.scale_t(kvs).to(DEV)
    cu0, cu1 = i32([0, prompt[0], sum(prompt)]), i32([0, 1, 2])
    need = plan(B, 1, Hq, topk, (torch.empty(P, page, DK), bt))[2]

    def state():
        s = dict(pool=torch.full((P, page, DK), NAN_BYTE, dtype=torch.uint8, device=DEV).view(F8), ipool=torch.zeros(P, page, 128, dtype=BF, device=DEV),
                 bt=bt.to(DEV), sl=i32(prompt), qo=torch.full((B, Hq, DK), Q_FILL, dtype=torch.int16, device=DEV).view(BF),
                 logits=torch.full((B, 1, ld), float("nan"), device=DEV), idx=torch.full((B, 1, topk), -9, dtype=torch.int32, device=DEV),
                 ws=torch.empty(max(need, 16), dtype=torch.uint8, device=DEV))
        s["o"], s["lse"] = outputs(B, 1, Hq)
        c.kv_append_paged_mla_bf16_fp8(c0.to(DEV), k0.to(DEV), s["pool"], s["bt"], s["sl"], cu0, sc, None, None, table, "interleaved")
        c.kv_append_paged_index_bf16(x0.to(DEV), s["ipool"], s["bt"], s["sl"], cu0)
        s["sl"].copy_(i32(lens))
        torch.cuda.synchronize()
        return s

    fixed = tuple(t.to(DEV) for t in (c1, k1, x1, q1, qi, wt))

    def step(s):
        c.kv_append_paged_mla_bf16_fp8(fixed[0], fixed[1], s["pool"], s["bt"], s["sl"], cu1, sc, fixed[3], s["qo"], table, "interleaved")
        c.kv_append_paged_index_bf16(fixed[2], s["ipool"], s["bt"], s["sl"], cu1)
        c.mla_index_logits_paged_bf16(fixed[4], fixed[5], s["ipool"], s["bt"], s["sl"], s["logits"])
        c.mla_index_topk(s["logits"], s["sl"], topk, s["idx"])
        c.fa2_decode_paged_mla_sparse_bf16_fp8(s["qo"].view(B, 1, Hq, DK), s["pool"], s["bt"], s["sl"], sc, s["idx"], SCALE, s["o"], s["lse"], s["ws"])

    e = state()
    step(e)
    torch.cuda.synchronize()
    pool, qo, idx, o, lse = (e[k].cpu() for k in ("pool", "qo", "idx", "o", "lse"))
    assert sorted(idx[1, 0].tolist()) == [-1] * (topk - lens[1]) + list(range(lens[1]))  # 8 visible keys: the dense list
    assert len(set(idx[0, 0].tolist())) == topk and all(0 <= p < lens[0] for p in idx[0, 0].tolist())  # 131 visible: 64 distinct positions
    ref = s8.decode_sparse(qo.view(B, 1, Hq, DK), pool, bt, lens, idx, kvs, SCALE)
    note("chain", check(o, lse, *ref, "mla sparse fp8 chain: append -> index append -> logits -> topk -> decode"))
    gs = state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(gs)
    torch.cuda.synchronize()
    assert bool((bits(gs["o"].cpu()) == O_FILL).all()) and bool((gs["idx"].cpu() == -9).all())  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gs["pool"].cpu().view(torch.uint8), pool.view(torch.uint8)) and torch.equal(gs["idx"].cpu(), idx)
    assert torch.equal(bits(gs["o"].cpu()), bits(o)) and torch.equal(fbits(gs["lse"].cpu()), fbits(lse))


# ---------------------------------------------------------------------------------------------------- 10. summary

def test_zz_summary_of_error_over_bound(built, dev):
    """The RATIOS table: the largest O err / bound of every group of parity cases of this file. Not an assertion of its own --
    every case asserted err <= bound where it ran."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
