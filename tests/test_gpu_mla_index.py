"""GPU: the DSA indexer -- cuda_learn_notes_amd.kv_append_paged_index_bf16, mla_index_logits_paged_bf16 and mla_index_topk
(csrc/kv_append_paged_index_bf16.*, csrc/mla_index_logits_paged_bf16.*, csrc/mla_index_topk.*) -- against
tests/mla_index_reference.py. The logits: within the derived bound 2^-23 (128 + 64 + 2) A of the fp64 reference, bit-exact where the answer
is exact, nothing written at or past vis or outside the tensor, nothing read behind the lengths (NaN in every unlisted pool row, NaN pages
behind the table entries past a sequence's pages, NaN behind q_idx and weights). The top-k: torch.equal with the exact reference, no
tolerance. Then independence, replay, 4-byte aligned operands, a captured graph of a whole V3.2 attention step, and the chain into
fa2_decode_paged_mla_sparse_bf16. Every parity case prints err / bound before it asserts (pytest -s); the last test prints the largest.

Also here: every head-block count of the logits kernel (Hi 32 ... 63), pages 32, 128 and 256, a negative length, and the edges of the
append's contract. The long rows of the top-k, the rows at every 4-byte residue and the pools and tensors past 2^32 elements are in
tests/test_gpu_mla_index_long_rows.py, _large_pool.py and _large_rows.py, which use this file's helpers.

Largest err / bound seen on an MI355X: see DESIGN 4.4.22 and profiles/r32_mla_index_tests.log, profiles/r34_mla_index_tests.log."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mla_index_reference as ix  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_gpu_paged_mla_sparse as ts  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENT, ISENT = 0x7FC12345, -7777  # a NaN pattern no kernel makes; an index no kernel writes
RATIOS = {}


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def ibits(x):
    return x.view(torch.int32)


def off4(t):
    """t on the device at data_ptr() % 16 == 4."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def run_logits(q, w, pool, bt, lens, ld, shift=False, tail_nan=False):
    """logits [B,T,ld] on the CPU, every entry pre-filled with SENT, inside guard bands that must keep SENT. shift: block_table, seqlens,
    weights and logits at 4 bytes past a 16-byte boundary. tail_nan: q_idx and weights sit at the end of allocations whose tail is NaN."""
    B, T = q.shape[:2]
    dv = "cuda"
    place = off4 if shift else (lambda t: t.to(dv))
    big = torch.full(((B + 2) * T * ld + 8,), SENT, dtype=torch.int32, device=dv).view(torch.float32)
    o = 1 if shift else 0
    lg = big[T * ld + o:T * ld + o + B * T * ld].view(B, T, ld)
    assert not shift or lg.data_ptr() % 16 == 4
    qd, wd = q.to(dv), place(w)
    if tail_nan:
        qb = torch.full((q.numel() + 16 * ix.D,), ix.NAN, dtype=BF, device=dv)
        wb = torch.full((w.numel() + 64,), ix.NAN, dtype=torch.float32, device=dv)
        qd, wd = qb[:q.numel()].view(q.shape), wb[:w.numel()].view(w.shape)
        qd.copy_(q), wd.copy_(w)
    pkg().mla_index_logits_paged_bf16(qd, wd, pool.to(dv), place(bt), place(torch.tensor(lens, dtype=torch.int32)), lg)
    torch.cuda.synchronize()
    flat = ibits(big).cpu()
    assert bool((flat[:T * ld + o] == SENT).all()) and bool((flat[T * ld + o + B * T * ld:] == SENT).all()), "guard bands of logits"
    return lg.cpu()


def check_logits(got, ref, bound, vis, label):
    worst = 0.0
    B, T, ld = got.shape
    for b in range(B):
        for t in range(T):
            n = max(vis[b][t], 0)
            assert bool((ibits(got[b, t, n:]) == SENT).all()), (label, b, t, "written at or past vis")
            if n:
                err = (got[b, t, :n].double() - ref[b, t, :n]).abs()
                assert bool(torch.isfinite(got[b, t, :n]).all()), (label, b, t)
                ok = err <= bound[b, t, :n]
                r = float((err / bound[b, t, :n].clamp_min(1e-300)).max())
                worst = max(worst, r)
                assert bool(ok.all()), (label, b, t, r)
    print("%s: largest err / bound %.4f" % (label, worst))
    RATIOS[label.split(":")[0]] = max(RATIOS.get(label.split(":")[0], 0.0), worst)
    return worst


def run_topk(logits, lens, topk, shift=False, ptrs=None):
    """indices [B,T,topk] on the CPU, pre-filled with ISENT inside guard bands that must keep it. ptrs: a list that receives data_ptr() of
    the logits on the device."""
    B, T, ld = logits.shape
    dv = "cuda"
    place = off4 if shift else (lambda t: t.to(dv))
    o = 1 if shift else 0
    big = torch.full(((B + 2) * T * topk + 8,), ISENT, dtype=torch.int32, device=dv)
    idx = big[T * topk + o:T * topk + o + B * T * topk].view(B, T, topk)
    assert not shift or idx.data_ptr() % 16 == 4
    ld_ = place(logits)
    if ptrs is not None:
        ptrs.append(ld_.data_ptr())
    pkg().mla_index_topk(ld_, place(torch.tensor(lens, dtype=torch.int32)), topk, idx)
    torch.cuda.synchronize()
    flat = big.cpu()
    assert bool((flat[:T * topk + o] == ISENT).all()) and bool((flat[T * topk + o + B * T * topk:] == ISENT).all()), "guard bands of indices"
    return idx.cpu()


# ---------------------------------------------------------------------------------------------------- 1. logits against the bound

def test_describe_names_the_three_head_block_kernel(built):
    """Hi = 33 ... 48 launch mla_index_logits_paged_bf16_mfma<3>; the shapes below are tested further down."""
    m = pkg().manifest
    for Hi, T, nhb in ((32, 3, 2), (33, 3, 3), (48, 1, 3), (49, 1, 4), (63, 3, 4)):
        text = m.describe_mla_index_logits_paged_bf16(len(ix.ONE_LENS), T, Hi, ix.ONE_NMAX, ix.ONE_NMAX // 16, 16)
        assert text.startswith("mla_index_logits_paged_bf16_mfma<NHB=%d> T=%d Hi=%d " % (nhb, T, Hi)), text[:80]


@pytest.mark.parametrize("HT", ix.ONE_HT_MORE, ids=lambda ht: "Hi%dxT%d" % ht)
def test_logits_within_the_bound_at_every_head_block_count(built, dev, HT):
    """Hi 32, 33, 48, 49, 63 at page 16: NHB = 2 (a full second block, no padding heads), 3, 3 (the instantiation no other test launches,
    at both of its ends), 4, 4; the bound is test_logits_within_the_bound's."""
    Hi, T = HT
    q, w, (pool, bt), lens, ld = ix.one_case(Hi, T, 16)
    ref, bound, vis = ix.reference("one", Hi, T, 16)
    check_logits(run_logits(q, w, pool, bt, lens, ld), ref, bound, vis, "logits head blocks: Hi=%d T=%d NHB=%d" % (Hi, T, -(-Hi // 16)))


@pytest.mark.parametrize("page", [32, 128, 256])
def test_logits_within_the_bound_at_the_other_pages(built, dev, page):
    """(Hi, T) = (17, 8) behind pages of 32, 128 and 256 rows (Nmax 320, 512, 4096): at page 256 the sixteen table entries a wave loads at
    once are one entry, and the sequence of 257 keys has one row in its second page."""
    Hi, T = ix.PAGED_HT
    q, w, (pool, bt), lens, ld = ix.paged_case(page)
    assert pool.shape[1] == page and bt.shape[1] * page == ld
    ref, bound, vis = ix.logits_ref(q, w, pool, bt, lens, ld)
    check_logits(run_logits(q, w, pool, bt, lens, ld), ref, bound, vis, "logits pages: Hi=%d T=%d page=%d" % (Hi, T, page))


@pytest.mark.parametrize("page", [32, 128, 256])
def test_logits_several_chunks_at_the_other_pages(built, dev, page):
    """long_case's problem (Nmax 4096, four chunks) behind pages of 32, 128 and 256 rows."""
    q, w, (pool, bt), lens, ld = ix.long_case_paged(page)
    ref, bound, vis = ix.logits_ref(q, w, pool, bt, lens, ld)
    check_logits(run_logits(q, w, pool, bt, lens, ld), ref, bound, vis, "logits several chunks, pages: page=%d" % page)


def test_logits_with_a_negative_length_writes_nothing_for_it(built, dev):
    """max(seqlens[b], 0): the sequence of length -5 keeps the sentinel in all of its rows; its neighbours are within the bound."""
    q, w, (pool, bt), lens, ld = ix.neg_case()
    assert lens[1] == -5
    ref, bound, vis = ix.logits_ref(q, w, pool, bt, lens, ld)
    assert all(v <= 0 for v in vis[1])
    got = run_logits(q, w, pool, bt, lens, ld)
    check_logits(got, ref, bound, vis, "logits negative length: Hi=17 T=3")
    assert bool((ibits(got[1]) == SENT).all())


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("HT", ix.ONE_HT, ids=lambda ht: "Hi%dxT%d" % ht)
def test_logits_within_the_bound(built, dev, HT, page):
    """Hi 1, 16, 17, 64 and T 1, 3, 8, 33 at the family's edge lengths 0, 1, 17, 63, 64, 65, 100, 257 (Nmax 320), weights of both signs; every
    j >= vis keeps the sentinel (a sequence with len 0 or vis <= 0 writes nothing), the guard bands too; the pool's unlisted rows and the
    pages behind the table entries past a sequence's pages hold NaN."""
    Hi, T = HT
    q, w, (pool, bt), lens, ld = ix.one_case(Hi, T, page)
    ref, bound, vis = ix.reference("one", Hi, T, page)
    check_logits(run_logits(q, w, pool, bt, lens, ld), ref, bound, vis, "logits one chunk: Hi=%d T=%d page=%d" % (Hi, T, page))


def test_logits_several_chunks_and_a_ragged_last_one(built, dev):
    """Nmax 4096, lengths 4000, 2048, 300, 100, 0, Hi 64, T 3: four chunks of 1024 keys, the last one ragged in its last wave and block."""
    q, w, (pool, bt), lens, ld = ix.long_case()
    ref, bound, vis = ix.reference("long")
    check_logits(run_logits(q, w, pool, bt, lens, ld), ref, bound, vis, "logits several chunks: Hi=64 T=3")


@pytest.mark.parametrize("ld", [100, 321, 5000])
def test_logits_cap_is_the_smaller_of_the_cache_and_ld(built, dev, ld):
    """ld below, just above and far above max_pages page = 320: cap = min(320, ld) clamps the lengths."""
    Hi, T, page = 17, 3, 16
    q, w, (pool, bt), lens, _ = ix.one_case(Hi, T, page)
    ref, bound, vis = ix.logits_ref(q, w, pool, bt, lens, ld)
    assert max(max(v) for v in vis) == min(ld, 257)
    check_logits(run_logits(q, w, pool, bt, lens, ld), ref, bound, vis, "logits cap: ld=%d" % ld)


# ---------------------------------------------------------------------------------------------------- 2. exact answers

def _exact(Hi, tail_nan=False):
    q, w, (pool, bt), lens, ld = ix.exact_case(Hi, 3, 16)
    ref, _, vis = ix.logits_ref(q, w, pool, bt, lens, ld)
    got = run_logits(q, w, pool, bt, lens, ld, tail_nan=tail_nan)
    for b in range(len(lens)):
        for t in range(q.shape[1]):
            n = max(vis[b][t], 0)
            assert torch.equal(got[b, t, :n].double(), ref[b, t, :n]), (Hi, b, t)
            assert bool((ibits(got[b, t, n:]) == SENT).all())


def test_logits_exact_integers(built, dev):
    """Integer q, k in [-4, 4] and weights +- 2^e: bit equality with the fp64 reference (tests/test_mla_index_surface.py proves that every
    partial sum stays below 2^24 quarter units)."""
    _exact(64)


@pytest.mark.parametrize("Hi", [48, 33])
def test_logits_exact_integers_on_three_head_blocks(built, dev, Hi):
    """The same at Hi = 48 and 33: both ends of mla_index_logits_paged_bf16_mfma<3>, the second with 15 padding heads."""
    _exact(Hi)


def test_logits_all_negative_products_are_plus_zero(built, dev):
    """Every head's dot product is negative: the logits are +0, bit for bit."""
    B, T, Hi = len(ix.ONE_LENS), 2, 17
    q = torch.ones(B, T, Hi, ix.D, dtype=BF)
    k = -torch.ones(B, ix.ONE_NMAX, ix.D, dtype=BF)
    w = torch.randn(B, T, Hi, generator=torch.Generator().manual_seed(1))
    pool, bt = ix.make_pool(k, 16, ix.ONE_LENS, seed=1)
    got = run_logits(q, w, pool, bt, ix.ONE_LENS, ix.ONE_NMAX)
    vis = ix.visible(ix.ONE_LENS, T, ix.ONE_NMAX)
    for b in range(B):
        for t in range(T):
            n = max(vis[b][t], 0)
            assert bool((ibits(got[b, t, :n]) == 0).all()) and bool((ibits(got[b, t, n:]) == SENT).all())


def test_logits_padding_heads_contribute_nothing(built, dev):
    """Hi = 17: the heads 17 ... 31 of the second block of 16 would read the bytes behind q_idx and weights, which hold NaN here."""
    _exact(17, tail_nan=True)


@pytest.mark.parametrize("Hi", [33, 49])
def test_logits_padding_heads_of_the_third_and_fourth_block(built, dev, Hi):
    """Hi = 33, 49: fifteen padding heads in the last of three and of four blocks, NaN behind q_idx and weights. The surface test's proof
    that every partial sum stays below 2^24 quarter units was written for Hi = 64; these cases sum over fewer heads, so it covers them (the
    surface test runs it at these Hi too)."""
    _exact(Hi, tail_nan=True)


# ---------------------------------------------------------------------------------------------------- 3. top-k, exact

@pytest.mark.parametrize("kind", ix.VALUE_SETS)
@pytest.mark.parametrize("topk", ix.TOPKS)
def test_topk_is_exact(built, dev, topk, kind):
    """A row per n in {0, 1, topk - 1, topk, topk + 1, 4095, 4096, 4097, 5000} (4096 = the kernel's scan block), NaN poison at every j >= n:
    all-equal rows, two values whose tie class straddles the scan-block edge, keys that differ in their lowest or highest 8 bits only,
    negatives / +-0 / +-inf / denormals, heavy ties. torch.equal with the reference."""
    logits, ns = ix.topk_case(topk, kind)
    got = run_topk(logits, ns, topk)
    want = ix.topk_ref(logits, ns, topk)
    assert torch.equal(got, want), [(n, int((got[b] != want[b]).sum())) for b, n in enumerate(ns)]


def test_topk_clamps_the_length_and_moves_the_edge_per_token(built, dev):
    """seqlens above ld are clamped to ld; T = 5: the edge moves per token, the first tokens of the short sequences see fewer than topk or
    no position."""
    B, T, ld, topk = 4, 5, 300, 64
    g = torch.Generator().manual_seed(3)
    logits = (torch.randint(-20, 21, (B, T, ld), generator=g).float() / 8).contiguous()
    lens = [1000, 300, 66, 3]
    got = run_topk(logits, lens, topk)
    assert torch.equal(got, ix.topk_ref(logits, lens, topk))
    assert got[3, 0].tolist() == [-1] * topk and got[3, 4].tolist() == [0, 1, 2] + [-1] * (topk - 3) and int(got[0, 0].min()) >= 0


def test_topk_with_nan_inside_the_row_stays_in_range(built, dev):
    """A caller's NaNs inside [0, n): every index is a distinct position in [0, n), ascending, and every slot is filled."""
    B, ld, topk, n = 3, 5000, 64, 4500
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(B, 1, ld, generator=g)
    logits[0, 0, :n:7] = ix.NAN
    logits[1, 0] = ix.NAN
    logits[2, 0, 100:4400] = -ix.NAN
    got = run_topk(logits, [n] * B, topk)
    for b in range(B):
        row = got[b, 0].tolist()
        assert all(0 <= p < n for p in row) and all(x < y for x, y in zip(row, row[1:])), b


# ---------------------------------------------------------------------------------------------------- 4. the append

def test_append_writes_its_rows_and_nothing_else(built, dev):
    """A ragged packed batch: 0, 1, 5 and 40 new tokens (the last two cross page edges), packed rows in front of and behind the sequences;
    every row bit-exact at its (page, slot), every other pool byte untouched."""
    page, max_pages, B = 16, 8, 4
    new, lens_after = [0, 1, 5, 40], [37, 1, 18, 100]
    g = torch.Generator().manual_seed(8)
    pool = torch.randn(B * max_pages + 2, page, ix.D, generator=g).to(BF)
    bt = torch.randperm(B * max_pages, generator=g).to(torch.int32).view(B, max_pages)
    cu = [2]
    for n in new:
        cu.append(cu[-1] + n)
    total = cu[-1] + 3
    k_new = torch.randn(total, ix.D, generator=g).to(BF)
    want = ix.append_ref(pool, bt, lens_after, cu, k_new)
    assert int((want.view(torch.int16) != pool.view(torch.int16)).any(dim=-1).sum()) == sum(new)
    dv = "cuda"
    pd = pool.to(dv)
    pkg().kv_append_paged_index_bf16(k_new.to(dv), pd, bt.to(dv), torch.tensor(lens_after, dtype=torch.int32, device=dv),
                                     torch.tensor(cu, dtype=torch.int32, device=dv))
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu().view(torch.int16), want.view(torch.int16))


def _run_append(p, shift=False):
    """The pool after the append on the device, inside a guard page on each side; every byte starts as ix.MARK. Returns (pool on the CPU,
    the two guard pages)."""
    dv = "cuda"
    place = off4 if shift else (lambda t: t.to(dv))
    page, P = p["page"], p["P"]
    whole = torch.full((P + 2, page, ix.D), ix.MARK, dtype=torch.int16, device=dv).view(BF)
    pd = whole[1:P + 1]
    assert pd.is_contiguous() and pd.data_ptr() % 16 == 0
    pkg().kv_append_paged_index_bf16(p["k_new"].to(dv), pd, place(p["bt"]), place(torch.tensor(p["lens"], dtype=torch.int32)),
                                     place(torch.tensor(p["cu"], dtype=torch.int32)))
    torch.cuda.synchronize()
    out = whole.cpu()
    return out[1:P + 1], out[[0, P + 1]]


@pytest.mark.parametrize("shift", [False, True], ids=["base0", "base4"])
@pytest.mark.parametrize("name", ix.APPEND_CASES)
def test_append_edges(built, dev, name, shift):
    """The contract of csrc/kv_append_paged_index_bf16.cuh, byte for byte against ix.append_ref, every other pool byte and the guard pages
    before and after the pool keeping their marker: pages of 32, 128, 256; empty sequences at the start, in the middle and at the end;
    B = 1 with one row; B = 37 with five sequences that have rows; packed rows in front of cu_q[0] and behind cu_q[B]; seqlens[b] < T_b
    (pos < 0) and seqlens[b] > Nmax (pos >= Nmax) write nothing; table entries -1 and P under live positions store nothing; cu_q with a
    negative first entry and a last entry past total_q -- the Python entry passes cu_q to the device unread, so the clamp that runs is the
    kernel's. base4: block_table, seqlens and cu_q 4 bytes past a 16-byte boundary."""
    p = ix.append_problem(name)
    start = torch.full((p["P"], p["page"], ix.D), ix.MARK, dtype=torch.int16).view(BF)
    want = ix.append_ref(start, p["bt"], p["lens"], p["cu"], p["k_new"])
    got, guards = _run_append(p, shift)
    assert bool((guards.view(torch.int16) == ix.MARK).all()), "guard pages of the pool"
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), name
    assert int((got.view(torch.int16) != ix.MARK).any(dim=-1).sum()) > 0


# ---------------------------------------------------------------------------------------------------- 5. independence, replay, alignment

def test_a_sequence_alone_two_calls_and_four_byte_operands(built, dev):
    Hi, T, page, topk = 17, 3, 16, 64
    q, w, (pool, bt), lens, ld = ix.one_case(Hi, T, page)
    base = run_logits(q, w, pool, bt, lens, ld)
    assert torch.equal(ibits(run_logits(q, w, pool, bt, lens, ld)), ibits(base))
    assert torch.equal(ibits(run_logits(q, w, pool, bt, lens, ld, shift=True)), ibits(base))
    for b in range(len(lens)):
        one = run_logits(q[b:b + 1].contiguous(), w[b:b + 1].contiguous(), pool, bt[b:b + 1].contiguous(), lens[b:b + 1], ld)
        assert torch.equal(ibits(one[0]), ibits(base[b])), b
    clean = torch.where(ibits(base) == SENT, torch.full_like(base, ix.NAN), base)  # NaN poison at every j >= vis
    idx = run_topk(clean, lens, topk)
    assert torch.equal(idx, ix.topk_ref(clean, lens, topk))
    assert torch.equal(run_topk(clean, lens, topk), idx) and torch.equal(run_topk(clean, lens, topk, shift=True), idx)
    for b in range(len(lens)):
        assert torch.equal(run_topk(clean[b:b + 1].contiguous(), lens[b:b + 1], topk)[0], idx[b]), b


# ---------------------------------------------------------------------------------------------------- 6. end to end

def _index_inputs(lens, T, Hi, Nmax, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    q = torch.randn(B, T, Hi, ix.D, generator=g).to(BF)
    w = (torch.randn(B, T, Hi, generator=g) * (Hi * ix.D) ** -0.5).float()
    keys = torch.randn(B, Nmax, ix.D, generator=g).to(BF)
    return q, w, keys


def _append_all(keys, lens, P, page, bt):
    """An index pool of NaNs behind the latent cache's table, filled by ONE append of every sequence's len_b keys; (pool on the device, the
    CPU reference of it)."""
    dv = "cuda"
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    k_new = torch.cat([keys[b, :n] for b, n in enumerate(lens)] + [torch.zeros(1, ix.D, dtype=BF)])
    pool = torch.full((P, page, ix.D), ix.NAN, dtype=BF)
    pd = pool.to(dv)
    pkg().kv_append_paged_index_bf16(k_new.to(dv), pd, bt.to(dv), torch.tensor(lens, dtype=torch.int32, device=dv),
                                     torch.tensor(cu, dtype=torch.int32, device=dv))
    torch.cuda.synchronize()
    want = ix.append_ref(pool, bt, lens, cu, k_new)
    assert torch.equal(pd.cpu().view(torch.int16), want.view(torch.int16))
    return pd, want


def test_chain_on_short_sequences_gives_the_dense_entrys_bits(built, dev):
    """Every length <= topk, T = 3: append -> logits -> top-k gives the dense list, and fa2_decode_paged_mla_sparse_bf16 on it gives O and LSE
    bit-equal to fa2_decode_paged_mla_bf16."""
    T, Hq, page, topk, Hi = 3, 5, 16, sp.ONE_NMAX, 16
    q, lens, (pool, bt) = sp.one_case(T, Hq, page)
    qi, w, keys = _index_inputs(lens, T, Hi, sp.ONE_NMAX, 21)
    _, ipool = _append_all(keys, lens, pool.shape[0], page, bt)
    lg = run_logits(qi, w, ipool, bt, lens, sp.ONE_NMAX)
    idx = run_topk(lg, lens, topk)
    assert torch.equal(idx, sp.dense_indices(lens, T, sp.ONE_NMAX, topk))
    assert ts.same(ts.sparse(q, (pool, bt), lens, idx), ts.dense(q, (pool, bt), lens))


def test_chain_on_long_sequences(built, dev):
    """Lengths 4000, 2048, 300, 100, 0 at topk 2048, T = 1, Hi = 64: the top-k of the kernel's own logits equals the top-k reference on those
    logits exactly; against the fp64 logits every selected position lies at or above tau - 2 bound and every unselected visible one at or
    below tau + 2 bound (tau the reference's topk-th value: the threshold moves by at most the bound of the position that sets it and each
    position by its own); the sparse decode on the list meets the family's o_bound against decode_sparse on the same list."""
    T, Hq, topk, Hi = 1, 16, 2048, 64
    q, lens, (pool, bt) = sp.split_case(T, Hq)
    page, Nmax = pool.shape[1], bt.shape[1] * pool.shape[1]
    qi, w, keys = _index_inputs(lens, T, Hi, Nmax, 22)
    _, ipool = _append_all(keys, lens, pool.shape[0], page, bt)
    lg = run_logits(qi, w, ipool, bt, lens, Nmax)
    ref, bound, vis = ix.logits_ref(qi, w, ipool, bt, lens, Nmax)
    check_logits(lg, ref, bound, vis, "logits chain: Hi=64 T=1")
    idx = run_topk(lg, lens, topk)
    assert torch.equal(idx, ix.topk_ref(lg, lens, topk))
    for b, n in enumerate(lens):
        if n <= topk:
            continue
        r, bd = ref[b, 0, :n], bound[b, 0, :n]
        tau = float(torch.sort(r, descending=True).values[topk - 1])
        chosen = torch.zeros(n, dtype=torch.bool)
        chosen[idx[b, 0].long()] = True
        assert int(chosen.sum()) == topk
        assert bool((r[chosen] >= tau - 2 * bd[chosen]).all()) and bool((r[~chosen] <= tau + 2 * bd[~chosen]).all()), b
    got = ts.sparse(q, (pool, bt), lens, idx)
    ts.check(*got, *ts.reference(q, (pool, bt), lens, idx), "mla sparse on the indexer's list, topk 2048")


def test_captured_graph_of_a_whole_step_replays_the_eager_bits(built, dev):
    """append of the latent rows' index keys -> logits -> top-k -> sparse decode, captured in one graph and replayed on fresh buffers: the
    logits, the list, O and LSE are the eager run's, bit for bit."""
    c = pkg()
    T, Hq, topk, Hi = 1, 16, 2048, 64
    q, lens, (pool, bt) = sp.split_case(T, Hq)
    page, Nmax, B = pool.shape[1], bt.shape[1] * pool.shape[1], len(lens)
    qi, w, keys = _index_inputs(lens, T, Hi, Nmax, 23)
    dv = "cuda"
    k_new = torch.stack([keys[b, max(n - 1, 0)] for b, n in enumerate(lens)]).to(dv)  # the newest token's key of every sequence
    cu = torch.tensor([0, 1, 2, 3, 4, 4], dtype=torch.int32, device=dv)               # the empty sequence appends nothing
    ipool0, _ = _append_all(keys, lens, pool.shape[0], page, bt)
    fixed = (q.to(dv), pool.to(dv), bt.to(dv), torch.tensor(lens, dtype=torch.int32, device=dv), qi.to(dv), w.to(dv))
    need = c.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, topk, bt.shape[1], page)[2]

    def buffers():
        return (ipool0.clone(), torch.full((B, T, Nmax), SENT, dtype=torch.int32, device=dv).view(torch.float32),
                torch.full((B, T, topk), ISENT, dtype=torch.int32, device=dv),
                torch.full((B, T, Hq, ml.DC), ts.O_FILL, dtype=torch.int16, device=dv).view(BF),
                torch.full((B, T, Hq), ts.L_FILL, dtype=torch.int32, device=dv).view(torch.float32), torch.empty(max(need, 16), dtype=torch.uint8, device=dv))

    def step(ipool, lg, idx, o, lse, ws):
        qd, pd, bd, sl, qid, wd = fixed
        c.kv_append_paged_index_bf16(k_new, ipool, bd, sl, cu)
        c.mla_index_logits_paged_bf16(qid, wd, ipool, bd, sl, lg)
        c.mla_index_topk(lg, sl, topk, idx)
        c.fa2_decode_paged_mla_sparse_bf16(qd, pd, bd, sl, idx, ml.SCALE, o, lse, ws)

    eager = buffers()
    step(*eager)
    torch.cuda.synchronize()
    bufs = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(*bufs)
    torch.cuda.synchronize()
    assert bool((bufs[2] == ISENT).all())  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ibits(bufs[1]), ibits(eager[1])) and torch.equal(bufs[2], eager[2])
    assert torch.equal(ts.bits(bufs[3].cpu()), ts.bits(eager[3].cpu())) and torch.equal(ts.fbits(bufs[4].cpu()), ts.fbits(eager[4].cpu()))
    assert torch.equal(eager[2].cpu(), ix.topk_ref(eager[1].cpu(), lens, topk))


# ---------------------------------------------------------------------------------------------------- 7. summary

def test_zz_summary_of_error_over_bound(built, dev):
    """The largest logit err / bound of every group of this file. Not an assertion of its own -- every case asserted
    err <= bound where it ran."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
