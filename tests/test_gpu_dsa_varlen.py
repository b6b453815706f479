"""GPU: the packed ("varlen") DSA step -- cuda_learn_notes_amd.mla_index_logits_paged_varlen_bf16[_fp8], mla_index_topk_varlen,
fa2_decode_paged_mla_sparse_varlen_bf16[_fp8] (csrc/dsa_varlen_row.cuh and the five *_varlen_* compile units).

No new tolerance. Every expectation is bit equality with the fixed-T entry, or the fixed-T entry's own reference with its own bound, sequence
by sequence (tests/dsa_varlen_reference.py): the logits within mla_index_reference's derived bound, the lists torch.equal, O within
paged_bf16_reference.o_bound of the emulation and LSE within decode_reference.lse_tol (test_gpu_paged_sink_attention.check).

The ragged batch is B = 7, T_b = (0, 1, 3, 0, 70, 2, 0) with two rows in front of cu_q[0] and three behind cu_q[B] (total_q = 81), vis
1023 / 1024 / 1025 at max_pages page = 2048, 0 / 1 / 2 and 31 ... 100. Outputs are pre-filled (O_FILL / L_FILL, a NaN pattern for the logits,
a marker for the lists) and stand between guard bands; the q rows of rows of no sequence are NaN; every unlisted pool row is NaN and every
table entry past a sequence's pages names a page of NaNs. Every parity case prints err / bound before it asserts (pytest -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsa_varlen_reference as dv  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DC, DK, SCALE, NMAX, PAGE, KVS = dv.DC, dv.DK, sp.SCALE, dv.NMAX, dv.PAGE, dv.KV_SCALE
O_FILL, L_FILL = sk.O_FILL, sk.L_FILL
LG_FILL, IX_MARK, WS_FILL = 0x7FC0A5A5, -77, 0x5A
NEG_INF = float("-inf")
G = 4  # guard rows on either side of every output
bits, fbits, check = sk.bits, sk.fbits, sk.check
RAGGED = (tuple(dv.RAGGED_LENS), tuple(dv.RAGGED_CU), dv.RAGGED_TOTAL)
SINGLE = (tuple(dv.SINGLE_LENS), tuple(dv.SINGLE_CU), dv.SINGLE_TOTAL)
EMPTY = (tuple(dv.EMPTY_LENS), tuple(dv.EMPTY_CU), dv.EMPTY_TOTAL)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def ints(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


def guarded(rows, shape, fill, dtype, view=None):
    """(whole, middle): a filled buffer of rows + 2 G rows and the view of its middle rows, which is what an entry gets."""
    whole = torch.full((rows + 2 * G,) + tuple(shape), fill, dtype=dtype, device="cuda")
    whole = whole.view(view) if view is not None else whole
    return whole, whole[G:G + rows]


def guards_untouched(whole, fill, as_int):
    w = whole.view(as_int).cpu()
    return bool((w[:G] == fill).all()) and bool((w[-G:] == fill).all())


def run_logits(fp8, q, w, pool, bt, lens, cu, ld=NMAX):
    """logits fp32 [total_q, ld] on the CPU; the guard bands asserted here."""
    c = pkg()
    total_q = q.shape[0]
    whole, lg = guarded(total_q, (ld,), LG_FILL, torch.int32, torch.float32)
    fn = c.mla_index_logits_paged_varlen_bf16_fp8 if fp8 else c.mla_index_logits_paged_varlen_bf16
    fn(q.cuda(), w.cuda(), pool.cuda(), bt.cuda(), ints(lens), ints(cu), lg)
    torch.cuda.synchronize()
    assert guards_untouched(whole, LG_FILL, torch.int32)
    return lg.cpu()


def run_logits_fixed(fp8, q, w, pool, bt, lens, ld=NMAX):
    c = pkg()
    B, T = q.shape[:2]
    lg = torch.full((B, T, ld), LG_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    fn = c.mla_index_logits_paged_bf16_fp8 if fp8 else c.mla_index_logits_paged_bf16
    fn(q.cuda(), w.cuda(), pool.cuda(), bt.cuda(), ints(lens), lg)
    torch.cuda.synchronize()
    return lg.cpu()


def run_topk(logits, lens, cu, topk):
    total_q = logits.shape[0]
    whole, idx = guarded(total_q, (topk,), IX_MARK, torch.int32)
    pkg().mla_index_topk_varlen(logits.cuda(), ints(lens), ints(cu), topk, idx)
    torch.cuda.synchronize()
    assert guards_untouched(whole, IX_MARK, torch.int32)
    return idx.cpu()


def run_topk_fixed(logits, lens, topk):
    B, T = logits.shape[:2]
    idx = torch.full((B, T, topk), IX_MARK, dtype=torch.int32, device="cuda")
    pkg().mla_index_topk(logits.cuda(), ints(lens), topk, idx)
    torch.cuda.synchronize()
    return idx.cpu()


def sparse_plan(total_q, Hq, topk):
    return pkg().fa2_decode_paged_mla_sparse_varlen_bf16_plan(total_q, Hq, topk, dv.MAX_PAGES, PAGE)


def run_sparse(fp8, q, pool, bt, lens, cu, idx):
    """(o, lse) on the CPU; o, lse and the workspace between guard bands, asserted here."""
    c = pkg()
    total_q, Hq, _ = q.shape
    need = sparse_plan(total_q, Hq, idx.shape[1])[2]
    ow, o = guarded(total_q, (Hq, DC), O_FILL, torch.int16, BF)
    lw, lse = guarded(total_q, (Hq,), L_FILL, torch.int32, torch.float32)
    wsw = torch.full((need + 512,), WS_FILL, dtype=torch.uint8, device="cuda")
    ws = wsw[256:256 + max(need, 16)]
    if fp8:
        c.fa2_decode_paged_mla_sparse_varlen_bf16_fp8(q.cuda(), pool.cuda(), bt.cuda(), ints(lens), ints(cu), torch.tensor([KVS], device="cuda"),
                                                      idx.cuda(), SCALE, o, lse, ws)
    else:
        c.fa2_decode_paged_mla_sparse_varlen_bf16(q.cuda(), pool.cuda(), bt.cuda(), ints(lens), ints(cu), idx.cuda(), SCALE, o, lse, ws)
    torch.cuda.synchronize()
    assert guards_untouched(ow, O_FILL, torch.int16) and guards_untouched(lw, L_FILL, torch.int32)
    wc = wsw.cpu()
    assert bool((wc[:256] == WS_FILL).all()) and bool((wc[256 + max(need, 16):] == WS_FILL).all())
    return o.cpu(), lse.cpu()


def run_sparse_fixed(fp8, q, pool, bt, lens, idx):
    c = pkg()
    B, T, Hq, _ = q.shape
    name = "fa2_decode_paged_mla_sparse_bf16" + ("_fp8" if fp8 else "")
    need = getattr(c, name + "_plan")(B, T, Hq, idx.shape[2], dv.MAX_PAGES, PAGE)[2]
    o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device="cuda").view(BF)
    lse = torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    more = (torch.tensor([KVS], device="cuda"),) if fp8 else ()
    getattr(c, name)(q.cuda(), pool.cuda(), bt.cuda(), ints(lens), *more, idx.cuda(), SCALE, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def check_logits(got, ref, bound, what):
    """Within the derived bound where the reference writes; the fill, bit for bit, everywhere else. Returns err / bound."""
    fin = torch.isfinite(ref)
    assert bool((fbits(got)[~fin] == LG_FILL).all()), what
    assert bool(torch.isfinite(got[fin]).all()), what
    err = (got.double()[fin] - ref[fin]).abs()
    ratio = float((err / bound[fin].clamp_min(1e-300)).max()) if int(fin.sum()) else 0.0
    print("%s: %d logits written, largest err / bound %.4f" % (what, int(fin.sum()), ratio))
    assert bool((err <= bound[fin]).all()), (what, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------- 1. the ragged batches, logits

@pytest.mark.parametrize("Hi", [1, 17, 64])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_logits_of_the_ragged_batch(built, dev, fp8, Hi):
    """Within the per-sequence reference's bound; nothing written past vis or in a row of no sequence, whose q and weights are NaN; and each
    sequence alone through the fixed-T entry with B = 1, T = T_b gives the bits of its packed rows."""
    lens, cu, total_q = RAGGED
    q, w = dv.index_queries(total_q, Hi, dv.no_sequence_rows(cu, total_q))
    pool, bt = dv.index_pool(lens, fp8)
    got = run_logits(fp8, q, w, pool, bt, lens, cu)
    ref, bound = dv.logits_ref(q, w, pool, bt, list(lens), list(cu), NMAX, fp8)
    written = [int(torch.isfinite(ref[r]).sum()) for r in range(total_q)]
    assert written[2] == 1023 and written[3:6] == [0, 1, 2] and written[76:78] == [1024, 1025] and sum(written[:2] + written[78:]) == 0
    check_logits(got, ref, bound, "varlen logits %s Hi=%d ragged" % ("fp8" if fp8 else "bf16", Hi))
    for b, c0, T in dv.sequences(list(cu), total_q):
        alone = run_logits_fixed(fp8, q[c0:c0 + T][None], w[c0:c0 + T][None], pool, bt[b:b + 1], [lens[b]])
        assert torch.equal(fbits(alone[0]), fbits(got[c0:c0 + T])), (b, T)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_logits_of_a_single_sequence_and_of_a_batch_without_a_token(built, dev, fp8):
    for lens, cu, total_q in (SINGLE, EMPTY):
        q, w = dv.index_queries(total_q, 17, dv.no_sequence_rows(cu, total_q))
        pool, bt = dv.index_pool(lens, fp8)
        got = run_logits(fp8, q, w, pool, bt, lens, cu)
        ref, bound = dv.logits_ref(q, w, pool, bt, list(lens), list(cu), NMAX, fp8)
        assert int(torch.isfinite(ref).sum()) == (38 + 39 + 40 if total_q == dv.SINGLE_TOTAL else 0)
        check_logits(got, ref, bound, "varlen logits %s B=1 total_q=%d" % ("fp8" if fp8 else "bf16", total_q))


# ---------------------------------------------------------------------------------------------------- 2. the ragged batches, top-k

def tie_logits(total_q, ld, seed=4):
    """fp32 [total_q, ld] with heavy ties: multiples of 1/4 in [0, 12)."""
    return (torch.randint(0, 48, (total_q, ld), generator=torch.Generator().manual_seed(seed)).float() / 4)


@pytest.mark.parametrize("topk", [64, 65, 2048])
def test_topk_of_the_ragged_batches(built, dev, topk):
    """torch.equal with the per-sequence reference; a row of no sequence all -1 though its logits are NaN; every sequence alone through the
    fixed-T entry gives the same lists."""
    for lens, cu, total_q in (RAGGED, SINGLE, EMPTY):
        lg = tie_logits(total_q, NMAX)
        vis = dv.vis_rows(lens, cu, total_q, NMAX)
        for r, v in enumerate(vis):
            lg[r, max(v or 0, 0):] = float("nan")  # not visible: never read
        got = run_topk(lg, lens, cu, topk)
        want = dv.topk_ref(lg, list(lens), list(cu), topk)
        assert torch.equal(got, want), (total_q, topk)
        for r in dv.no_sequence_rows(cu, total_q):
            assert bool((got[r] == -1).all())
        for b, c0, T in dv.sequences(list(cu), total_q):
            assert torch.equal(run_topk_fixed(lg[c0:c0 + T][None], [lens[b]], topk)[0], got[c0:c0 + T]), (b, T)
        # in the ragged batch the select ran, not only the dense list
        assert total_q != dv.RAGGED_TOTAL or topk == 2048 or (int((want[76] >= 0).sum()) == topk and want[76].tolist() != list(range(topk)))


# ---------------------------------------------------------------------------------------------------- 3. the ragged batches, sparse decode

@pytest.mark.parametrize("topk", [64, 65, 2048])
@pytest.mark.parametrize("Hq", [1, 17, 65, 128])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_sparse_decode_of_the_ragged_batch(built, dev, fp8, Hq, topk):
    """Within the per-sequence reference's bounds; rows of no sequence O = 0, LSE = -inf although their q is NaN and their lists name
    positions 0 ... topk - 1; one split at topk 64 and 65, several at 2048."""
    lens, cu, total_q = RAGGED
    S = sparse_plan(total_q, Hq, topk)[0]
    assert (S > 1) == (topk == 2048), S
    nos = dv.no_sequence_rows(cu, total_q)
    q = dv.latent_queries(total_q, Hq, nos, 32 if fp8 else 1)
    pool, bt = dv.latent_pool(lens, fp8)
    idx = dv.packed_indices(lens, cu, total_q, topk)
    o, lse = run_sparse(fp8, q, pool, bt, lens, cu, idx)
    ro, rl, emul = dv.sparse_ref(q, pool, bt, list(lens), list(cu), idx, SCALE, KVS if fp8 else None)
    for r in nos + (3,):  # row 3: vis = 0, a token of a sequence that sees no key
        assert bool((rl[r] == NEG_INF).all())
        assert bool((bits(o[r]) == 0).all()) and bool((lse[r] == NEG_INF).all()), r
    assert bool(torch.isfinite(rl[4]).all()) and bool(torch.isfinite(rl[77]).all())
    check(o, lse, ro, rl, emul, "varlen sparse %s Hq=%d topk=%d S=%d ragged" % ("fp8" if fp8 else "bf16", Hq, topk, S))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_sparse_decode_of_each_sequence_alone_is_bit_equal(built, dev, fp8):
    """topk 64: the packed plan and the plan of every sequence alone are one split, and the fixed-T entry with B = 1, T = T_b gives the bits
    of the sequence's packed rows. Also B = 1 and the batch without a token."""
    c = pkg()
    Hq, topk = 17, 64
    for lens, cu, total_q in (RAGGED, SINGLE, EMPTY):
        nos = dv.no_sequence_rows(cu, total_q)
        q = dv.latent_queries(total_q, Hq, nos)
        pool, bt = dv.latent_pool(lens, fp8)
        idx = dv.packed_indices(lens, cu, total_q, topk)
        S, C, _ = sparse_plan(total_q, Hq, topk)
        o, lse = run_sparse(fp8, q, pool, bt, lens, cu, idx)
        for r in nos:
            assert bool((bits(o[r]) == 0).all()) and bool((lse[r] == NEG_INF).all()), r
        for b, c0, T in dv.sequences(list(cu), total_q):
            assert c.fa2_decode_paged_mla_sparse_bf16_plan(1, T, Hq, topk, dv.MAX_PAGES, PAGE)[:2] == (S, C) == (1, 64)
            ao, al = run_sparse_fixed(fp8, q[c0:c0 + T][None], pool, bt[b:b + 1], [lens[b]], idx[c0:c0 + T][None])
            assert torch.equal(bits(ao[0]), bits(o[c0:c0 + T])) and torch.equal(fbits(al[0]), fbits(lse[c0:c0 + T])), (b, T)


# ---------------------------------------------------------------------------------------------------- 4. uniform offsets: the fixed-T bits

UNIFORM_LENS = {5: (1023, 2, 100, 1025, 0), 3: (1025, 3, 100), 2: (1060, 100)}


@pytest.mark.parametrize("BT", dv.UNIFORM_BT, ids=lambda bt: "B%dxT%d" % bt)
def test_uniform_offsets_give_the_bits_of_the_fixed_t_entries(built, dev, BT):
    """cu_q = [0, T, ..., B T]: all five packed entries against the fixed-T entries on the same tensors, the sparse pair at one split and at
    the several splits of topk 2048 (the plans asserted equal first)."""
    c = pkg()
    B, T = BT
    lens, cu, total_q = UNIFORM_LENS[B], tuple(dv.uniform_cu(B, T)), B * T
    for fp8 in (False, True):
        q, w = dv.index_queries(total_q, 17)
        pool, bt = dv.index_pool(lens, fp8)
        got = run_logits(fp8, q, w, pool, bt, lens, cu)
        want = run_logits_fixed(fp8, q.view(B, T, 17, dv.D), w.view(B, T, 17), pool, bt, lens)
        assert torch.equal(fbits(got), fbits(want.view(total_q, NMAX))) and int(torch.isfinite(got).sum()) > 0
    lg = tie_logits(total_q, NMAX)
    for topk in (64, 2048):
        assert torch.equal(run_topk(lg, lens, cu, topk), run_topk_fixed(lg.view(B, T, NMAX), lens, topk).view(total_q, topk))
    for fp8 in (False, True):
        pool, bt = dv.latent_pool(lens, fp8)
        for Hq, topk in ((17, 64), (128, 2048)):
            plan = sparse_plan(total_q, Hq, topk)
            assert plan == c.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, topk, dv.MAX_PAGES, PAGE) and (plan[0] > 1) == (topk == 2048)
            q = dv.latent_queries(total_q, Hq)
            idx = dv.packed_indices(lens, cu, total_q, topk)
            o, lse = run_sparse(fp8, q, pool, bt, lens, cu, idx)
            fo, fl = run_sparse_fixed(fp8, q.view(B, T, Hq, DK), pool, bt, lens, idx.view(B, T, topk))
            assert torch.equal(bits(o), bits(fo.view(total_q, Hq, DC))) and torch.equal(fbits(lse), fbits(fl.view(total_q, Hq))), (fp8, Hq, topk)
            assert bool(torch.isfinite(lse).any())


# ---------------------------------------------------------------------------------------------------- 5. malformed offsets

@pytest.mark.parametrize("kind", sorted(dv.MALFORMED))
def test_malformed_offsets_complete_and_leave_the_guard_bands_alone(built, dev, kind):
    """Decreasing, negative and too large offsets are outside the contract: the five entries still complete, touch nothing outside rows
    0 ... total_q - 1 (the guard bands, asserted by the runners), and every list slot of every row is written."""
    lens, _, total_q = RAGGED
    cu = tuple(dv.MALFORMED[kind])
    for fp8 in (False, True):
        q, w = dv.index_queries(total_q, 17)
        run_logits(fp8, q, w, *dv.index_pool(lens, fp8), lens, cu)
        idx = dv.packed_indices(lens, RAGGED[1], total_q, 2048)
        o, lse = run_sparse(fp8, dv.latent_queries(total_q, 17), *dv.latent_pool(lens, fp8), lens, cu, idx)
        assert not bool((bits(o) == O_FILL).all(dim=-1).any()) and not bool((fbits(lse) == L_FILL).any())  # every row written
    got = run_topk(tie_logits(total_q, NMAX), lens, cu, 64)
    assert not bool((got == IX_MARK).any())
    if kind != "decreasing":  # monotone after the clamp: the definition holds, and so does the reference
        assert torch.equal(got, dv.topk_ref(tie_logits(total_q, NMAX), list(lens), list(cu), 64))


# ---------------------------------------------------------------------------------------------------- 6. the chain and a captured graph

def _step_tensors(lens, cu, total_q, Hi, Hq, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(k_idx=torch.randn(total_q, dv.D, generator=g).to(BF), c_new=(torch.randn(total_q, DC, generator=g) * SCALE).to(BF),
                k_pe=(torch.randn(total_q, DK - DC, generator=g) * SCALE).to(BF), q_idx=torch.randn(total_q, Hi, dv.D, generator=g).to(BF),
                w=(torch.randn(total_q, Hi, generator=g) * (Hi * dv.D) ** -0.5).float(), q=(torch.randn(total_q, Hq, DK, generator=g) * SCALE).to(BF))


def _pools(B, seed):
    """Caches that hold finite history everywhere (identity-like shuffled tables): the step appends behind it."""
    g = torch.Generator().manual_seed(seed)
    P = B * dv.MAX_PAGES
    perm = torch.randperm(P, generator=g).to(torch.int32).view(B, dv.MAX_PAGES)
    return torch.randn(P, PAGE, dv.D, generator=g).to(BF), (torch.randn(P, PAGE, DK, generator=g) * SCALE).to(BF), perm


def _packed_step(c, t, idx_pool, pool, bt, sl, cu, bufs, topk):
    """append -> logits -> top-k -> sparse decode: four packed calls (the two appends are the step's first call on either cache)."""
    lg, ix_, o, lse, ws = bufs
    c.kv_append_paged_index_bf16(t["k_idx"], idx_pool, bt, sl, cu)
    c.kv_append_paged_mla_bf16(t["c_new"], t["k_pe"], pool, bt, sl, cu)
    c.mla_index_logits_paged_varlen_bf16(t["q_idx"], t["w"], idx_pool, bt, sl, cu, lg)
    c.mla_index_topk_varlen(lg, sl, cu, topk, ix_)
    c.fa2_decode_paged_mla_sparse_varlen_bf16(t["q"], pool, bt, sl, cu, ix_, SCALE, o, lse, ws)


def _bufs(total_q, Hq, topk):
    need = sparse_plan(total_q, Hq, topk)[2]
    return (torch.full((total_q, NMAX), LG_FILL, dtype=torch.int32, device="cuda").view(torch.float32),
            torch.full((total_q, topk), IX_MARK, dtype=torch.int32, device="cuda"),
            torch.full((total_q, Hq, DC), O_FILL, dtype=torch.int16, device="cuda").view(BF),
            torch.full((total_q, Hq), L_FILL, dtype=torch.int32, device="cuda").view(torch.float32),
            torch.empty(max(need, 16), dtype=torch.uint8, device="cuda"))


def test_the_packed_chain_equals_the_per_sequence_fixed_t_chain(built, dev):
    """The ragged batch through append -> packed logits -> packed top-k -> packed sparse decode, against each sequence alone through the
    fixed-T entries on the same caches: lists and O / LSE bit for bit (topk 64: one split either way)."""
    c = pkg()
    lens, cu, total_q = RAGGED
    Hi, Hq, topk = 17, 17, 64
    t = {k: v.cuda() for k, v in _step_tensors(lens, cu, total_q, Hi, Hq, 21).items()}
    idx_pool, pool, bt = (x.cuda() for x in _pools(len(lens), 22))
    sl, cud = ints(lens), ints(cu)
    bufs = _bufs(total_q, Hq, topk)
    _packed_step(c, t, idx_pool, pool, bt, sl, cud, bufs, topk)
    torch.cuda.synchronize()
    lg, ix_, o, lse = (x.cpu() for x in bufs[:4])
    for b, c0, T in dv.sequences(list(cu), total_q):
        s = slice(c0, c0 + T)
        alone = run_logits_fixed(False, t["q_idx"][s][None].cpu(), t["w"][s][None].cpu(), idx_pool.cpu(), bt[b:b + 1].cpu(), [lens[b]])
        assert torch.equal(fbits(alone[0]), fbits(lg[s])), b
        lists = run_topk_fixed(alone, [lens[b]], topk)
        assert torch.equal(lists[0], ix_[s]), b
        ao, al = run_sparse_fixed(False, t["q"][s][None].cpu(), pool.cpu(), bt[b:b + 1].cpu(), [lens[b]], lists)
        assert torch.equal(bits(ao[0]), bits(o[s])) and torch.equal(fbits(al[0]), fbits(lse[s])), b
    assert int((ix_[75] >= 0).sum()) == topk and bool(torch.isfinite(lse[75]).all())
    for r in dv.no_sequence_rows(cu, total_q):
        assert bool((ix_[r] == -1).all()) and bool((bits(o[r]) == 0).all()) and bool((lse[r] == NEG_INF).all())
        assert bool((fbits(lg[r]) == LG_FILL).all())


def test_a_captured_graph_of_the_packed_step_follows_the_offsets_on_the_device(built, dev):
    """The four-call packed step captured once; cu_q and seqlens then change ON THE DEVICE between replays (the ragged batch, then seven
    sequences of 12 and 9 tokens in the same 81 rows) and each replay gives the bits of the eager step on the same state."""
    c = pkg()
    lens, cu, total_q = RAGGED
    Hi, Hq, topk = 17, 65, 2048
    assert sparse_plan(total_q, Hq, topk)[0] > 1
    t = {k: v.cuda() for k, v in _step_tensors(lens, cu, total_q, Hi, Hq, 31).items()}
    idx0, pool0, bt = (x.cuda() for x in _pools(len(lens), 32))
    second = ((900, 901, 64, 17, 1500, 1, 2048), (0, 12, 24, 36, 48, 60, 72, 81))
    eager = []
    for ln, cq in ((lens, cu), second):
        idx_pool, pool, bufs = idx0.clone(), pool0.clone(), _bufs(total_q, Hq, topk)
        _packed_step(c, t, idx_pool, pool, bt, ints(ln), ints(cq), bufs, topk)
        torch.cuda.synchronize()
        eager.append([x.cpu() for x in bufs[:4]] + [idx_pool.cpu(), pool.cpu()])
    assert not torch.equal(eager[0][1], eager[1][1])
    idx_pool, pool, bufs = idx0.clone(), pool0.clone(), _bufs(total_q, Hq, topk)
    sl, cud = ints(lens), ints(cu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _packed_step(c, t, idx_pool, pool, bt, sl, cud, bufs, topk)
    torch.cuda.synchronize()
    assert bool((bits(bufs[2].cpu()) == O_FILL).all())  # captured, not run
    for (ln, cq), want in zip(((lens, cu), second), eager):
        idx_pool.copy_(idx0), pool.copy_(pool0), sl.copy_(ints(ln)), cud.copy_(ints(cq))
        for x, fill in zip(bufs[:4], (LG_FILL, IX_MARK, O_FILL, L_FILL)):
            x.view(torch.int16 if x.dtype == BF else torch.int32).fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        got = [x.cpu() for x in bufs[:4]] + [idx_pool.cpu(), pool.cpu()]
        assert torch.equal(fbits(got[0]), fbits(want[0])) and torch.equal(got[1], want[1])
        assert torch.equal(bits(got[2]), bits(want[2])) and torch.equal(fbits(got[3]), fbits(want[3]))
        assert torch.equal(bits(got[4]), bits(want[4])) and torch.equal(bits(got[5]), bits(want[5]))
