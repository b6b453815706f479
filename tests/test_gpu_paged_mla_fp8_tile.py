"""GPU: the latent cache in DeepSeek-V3.2's own FP8 row of 656 bytes (csrc/*_fp8_tile.*; DESIGN 4.4.26 has the largest err / bound seen): the
append against the fp32 formula on the CPU, the decode against the BITS of fa2_decode_paged_mla_sparse_bf16 on the pool dequantised by torch
and against fp64 under paged_mla_sparse_reference's bound, exact counts, surroundings, the packed form, the chain of four calls."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsa_varlen_reference as dv  # noqa: E402
import paged_edge_cases as ec  # noqa: E402
import paged_mla_fp8_tile_reference as tr  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_gpu_paged_mla_sparse as gs  # noqa: E402  (sparse(): the bf16 entry; same, check, the graph helper, the fills)
pytestmark = pytest.mark.gpu

BF, DC, DK, SCALE, NEG_INF = torch.bfloat16, sp.DC, sp.DK, sp.SCALE, float("-inf")
O_FILL, L_FILL, bits, fbits, same, pkg = gs.O_FILL, gs.L_FILL, gs.bits, gs.fbits, gs.same, gs.pkg


def outputs(*lead):
    return (torch.full((*lead, DC), O_FILL, dtype=torch.int16, device="cuda").view(BF),
            torch.full(lead, L_FILL, dtype=torch.int32, device="cuda").view(torch.float32))


def off4(t):
    v = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")[1:1 + t.numel()].view(t.shape).copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def tile(q, pool, lens, idx, cu=None):
    """(o, lse) of the new entry, computed on the GPU and copied back; cu: the packed entry. The int operands sit at data_ptr() % 16 == 4."""
    c, (o, lse) = pkg(), outputs(*q.shape[:-1])
    ints = [off4(pool[1]), off4(torch.tensor(list(lens), dtype=torch.int32))] + ([] if cu is None else [off4(torch.tensor(list(cu), dtype=torch.int32))])
    fn = c.fa2_decode_paged_mla_sparse_bf16_fp8_tile if cu is None else c.fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile
    fn(q.cuda(), pool[0].cuda(), *ints, off4(idx), SCALE, o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


APPEND_T, APPEND_LENS, APPEND_FRONT, APPEND_BACK = (3, 0, 20, 1), [5, 7, 70, 33], 1, 2  # T_b = 0; positions 50 ... 69 cross a page edge


@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("rope", ["none", "half"])
@pytest.mark.parametrize("page", [16, 64])
def test_append_writes_the_formula_bit_for_bit_and_nothing_else(built, dev, page, rope, pow2):
    c = pkg()
    cu = [APPEND_FRONT + sum(APPEND_T[:b]) for b in range(len(APPEND_T) + 1)]
    total_q, B, Hq, max_pages = cu[-1] + APPEND_BACK, len(APPEND_T), 3, 128 // page
    c_new, k_pe_new = (t.clone() for t in tr.latent(total_q, 21))
    c_new[2, :128] = 0                                        # an all-zero tile: scale = 1e-4 / 448, codes 0
    c_new[5, 128:256] = c_new[5, 128:256].clamp(-50, 50)
    c_new[5, 200] = 56.0                                      # a tile whose amax is exactly 448 * 2^-3
    q = torch.randn(total_q, Hq, DK, generator=torch.Generator().manual_seed(3)).to(BF)
    bt = torch.randperm(B * max_pages, generator=torch.Generator().manual_seed(page)).to(torch.int32).view(B, max_pages)
    P, pool = B * max_pages + 1, torch.full((B * max_pages + 1, page, tr.ROW), 0xA5, dtype=torch.uint8)
    table = None if rope == "none" else c.kv_append_rope_table(128, 64).cuda()
    dev_args = (bt.cuda(), torch.tensor(APPEND_LENS, dtype=torch.int32).cuda(), torch.tensor(cu, dtype=torch.int32).cuda())
    got, q_out = pool.cuda(), torch.full_like(q, 7.0).cuda()
    c.kv_append_paged_mla_bf16_fp8_tile(c_new.cuda(), k_pe_new.cuda(), got, *dev_args, q.cuda(), q_out, table, rope, pow2)
    sib, sib_q = torch.full((P, page, DK), 0, dtype=BF).view(torch.int16).fill_(-0x5A5B).view(BF).cuda(), torch.full_like(q, 7.0).cuda()
    c.kv_append_paged_mla_bf16(c_new.cuda(), k_pe_new.cuda(), sib, *dev_args, q.cuda(), sib_q, table, rope)
    torch.cuda.synchronize()
    want = tr.append_ref(pool, bt, APPEND_LENS, cu, c_new, k_pe_new, pow2)  # its k_pe is not looked at: the sibling's bits are
    for g, w in list(zip(tr.views(got.cpu()), tr.views(want)))[:2]:  # codes, scales
        assert torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8))
    assert torch.equal(bits(tr.views(got.cpu())[2].contiguous()), bits(sib.cpu()[..., DC:].contiguous()))  # untouched rows: 0xA5A5 in both
    assert torch.equal(bits(q_out.cpu()), bits(sib_q.cpu()))


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("TH", tr.TH, ids=lambda th: "T%dxHq%d" % th)
def test_decode_gives_the_bits_of_the_bf16_entry_on_the_dequantised_pool(built, dev, TH, page):
    """Fails without the feature and pins the scale placement; at the corners also the fp64 reference under the bf16 entry's bound."""
    T, Hq = TH
    for topk in tr.TOPKS:
        q, lens, pool, idx = tr.case(T, Hq, page, topk)
        S = pkg().fa2_decode_paged_mla_sparse_bf16_fp8_tile_plan(len(lens), T, Hq, topk, pool[1].shape[1], page)[0]
        assert (S > 1) == (topk == 1024) and S == gs.plan(len(lens), T, Hq, topk, pool)[0]
        got = tile(q, pool, lens, idx)
        assert same(got, gs.sparse(q, (tr.dequantised(pool[0]), pool[1]), lens, idx)), (T, Hq, page, topk)
        assert bool((bits(got[0][0]) == 0).all()) and bool((got[1][0] == NEG_INF).all())  # length 0
        if (T, Hq, page, topk) in tr.CORNERS:
            gs.check(*got, *sp.decode_sparse(q, tr.dequantised(pool[0]), pool[1], lens, idx, SCALE), "mla sparse fp8 tile T=%d Hq=%d page=%d topk=%d" % (T, Hq, page, topk))


@pytest.mark.parametrize("topk", [320, 1024], ids=["one-split", "several-splits"])
def test_exact_counts_with_empty_slots_in_front_of_a_nan_page(built, dev, topk):
    """q = 0, c = 1: O = 1, LSE = ln n; the n valid slots on 0, 63, 64, chunk - 1, chunk, topk - 1 in that order, the others -1, vis or Nmax + 5."""
    T, Hq, page, Nmax, length, edges = 2, 5, 16, 512, 300, (0, 63, 64, 255, 256, topk - 1)
    counts, lens = list(range(1, len(edges) + 1)), [length] * len(edges)
    idx = torch.tensor([-1, 0, Nmax + 5], dtype=torch.int32).repeat(len(counts), T, topk)[..., :topk].contiguous()
    for b, n in enumerate(counts):
        for t in range(T):
            idx[b, t][idx[b, t] == 0] = length - (T - 1 - t)  # vis itself
            idx[b, t, list(edges[:n])] = torch.arange(7 * b + t, 7 * b + t + n, dtype=torch.int32)
    c = torch.ones(len(counts), Nmax, DC, dtype=BF)
    k_pe = tr.latent(len(counts) * Nmax, 9)[1].view(len(counts), Nmax, tr.DR)
    pool = tr.listed_pool(c, k_pe, page, lens, tr.listed(lens, T, Nmax, idx), seed=topk)
    assert (pkg().fa2_decode_paged_mla_sparse_bf16_fp8_tile_plan(len(counts), T, Hq, topk, Nmax // page, page)[0] > 1) == (topk == 1024)
    o, lse = tile(torch.zeros(len(counts), T, Hq, DK, dtype=BF), pool, lens, idx)
    for b, n in enumerate(counts):
        assert bool((o[b] == 1).all()) and (lse[b].double() - math.log(n)).abs().max().item() <= ec.lse_tol_at(n), (b, n)


def test_guard_bands_and_a_captured_graph(built, dev):
    c = pkg()
    T, Hq, page, topk = 2, 40, 16, 1024
    q, lens, pool, idx = tr.case(T, Hq, page, topk)
    B, base = len(lens), tile(q, pool, lens, idx)
    need = c.fa2_decode_paged_mla_sparse_bf16_fp8_tile_plan(B, T, Hq, topk, pool[1].shape[1], page)[2]
    band, (big_o, big_l) = 4096, outputs(B + 2, T, Hq)
    big_w = torch.full((need + 2 * band,), 0x5A, dtype=torch.uint8, device="cuda")
    fixed = (q.cuda(), pool[0].cuda(), pool[1].cuda(), torch.tensor(lens, dtype=torch.int32).cuda(), idx.cuda(), SCALE)
    c.fa2_decode_paged_mla_sparse_bf16_fp8_tile(*fixed, big_o[1:B + 1], big_l[1:B + 1], big_w[band:band + need])
    torch.cuda.synchronize()
    assert same((big_o[1:B + 1].cpu(), big_l[1:B + 1].cpu()), base)
    for edge in (0, B + 1):
        assert bool((bits(big_o[edge].cpu()) == O_FILL).all()) and bool((fbits(big_l[edge].cpu()) == L_FILL).all())
    assert bool((big_w[:band] == 0x5A).all()) and bool((big_w[band + need:] == 0x5A).all())
    assert same(gs._graph_replays_eager(lambda o, lse, ws: c.fa2_decode_paged_mla_sparse_bf16_fp8_tile(*fixed, o, lse, ws), B, T, Hq, need), base)


@pytest.mark.parametrize("case", [(1, 16, 16, 130), (2, 40, 64, 1024)], ids=lambda c: "T%dxHq%d-page%d-topk%d" % c)
def test_packed_on_uniform_offsets_gives_the_bits_of_the_fixed_t_entry(built, dev, case):
    T, Hq, page, topk = case
    q, lens, pool, idx = tr.case(*case)
    B = len(lens)
    got = tile(q.view(B * T, Hq, DK), pool, lens, idx.view(B * T, topk), cu=dv.uniform_cu(B, T))
    want = tile(q, pool, lens, idx)
    assert same(got, (want[0].view(B * T, Hq, DC), want[1].view(B * T, Hq)))


def test_packed_ragged_batch_is_the_fixed_t_entry_per_sequence(built, dev):
    """T_b = (0, 1, 3, 0, 70, 2, 0), two rows in front and three behind; rows of no sequence list valid-looking positions: O = 0, LSE = -inf."""
    Hq, topk, cu, total_q, lens, B = 5, 64, dv.RAGGED_CU, dv.RAGGED_TOTAL, dv.RAGGED_LENS, len(dv.RAGGED_LENS)
    q = dv.latent_queries(total_q, Hq, mult=4)
    idx = dv.packed_indices(tuple(lens), tuple(cu), total_q, topk)
    vis = dv.vis_rows(lens, cu, total_q, dv.NMAX)
    pos = [sorted({p for r, row in enumerate(dv.rows(cu, total_q)) if row and row[0] == b for _, p in sp.valid_slots(idx[r], vis[r])}) for b in range(B)]
    c, k_pe = tr.latent(B * dv.NMAX, 13)
    pool = tr.listed_pool(c.view(B, dv.NMAX, DC), k_pe.view(B, dv.NMAX, tr.DR), dv.PAGE, lens, pos, seed=2)
    got = tile(q, pool, lens, idx, cu=cu)
    for r in dv.no_sequence_rows(tuple(cu), total_q):
        assert bool((bits(got[0][r]) == 0).all()) and bool((got[1][r] == NEG_INF).all()), r
    for b, c0, T in dv.sequences(cu, total_q):
        one = tile(q[c0:c0 + T][None].contiguous(), (pool[0], pool[1][b:b + 1].contiguous()), lens[b:b + 1], idx[c0:c0 + T][None].contiguous())
        assert same((got[0][c0:c0 + T][None], got[1][c0:c0 + T][None]), one), b


def test_the_four_call_step_on_the_models_two_cache_formats(built, dev):
    """A ragged prompt step (T_b = len_b = 40, 0, 100); O against the fp64 reference on the views of the pool the append wrote."""
    c = pkg()
    lens, cu, page, max_pages, Hq, Hi, topk = [40, 0, 100], [0, 40, 40, 140], 16, 8, 16, 4, 32
    total_q, B, g = cu[-1], len(lens), torch.Generator().manual_seed(4)
    c_new, k_pe_new = tr.latent(total_q, 17)
    k_idx, q_idx = (torch.randn(*s, generator=g).to(BF) for s in ((total_q, 128), (total_q, Hi, 128)))
    w = (torch.randn(total_q, Hi, generator=g) * 0.05).float()
    q = dv.latent_queries(total_q, Hq, mult=4)
    bt = torch.randperm(B * max_pages, generator=g).to(torch.int32).view(B, max_pages)
    pool, idx_pool = tr.nan_pool(B * max_pages, page).cuda(), torch.zeros(B * max_pages, page, 132, dtype=torch.uint8).cuda()
    ints = (bt.cuda(), torch.tensor(lens, dtype=torch.int32).cuda(), torch.tensor(cu, dtype=torch.int32).cuda())
    c.kv_append_paged_mla_bf16_fp8_tile(c_new.cuda(), k_pe_new.cuda(), pool, *ints, scale_pow2=True)
    c.kv_append_paged_index_bf16_fp8(k_idx.cuda(), idx_pool, *ints, scale_pow2=True)
    logits = torch.zeros(total_q, max_pages * page, device="cuda")
    c.mla_index_logits_paged_varlen_bf16_fp8(q_idx.cuda(), w.cuda(), idx_pool, *ints, logits)
    idx = torch.zeros(total_q, topk, dtype=torch.int32, device="cuda")
    c.mla_index_topk_varlen(logits, ints[1], ints[2], topk, idx)
    o, lse = outputs(total_q, Hq)
    c.fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile(q.cuda(), pool, *ints, idx, SCALE, o, lse)
    torch.cuda.synchronize()
    assert int((idx.cpu() >= 0).sum()) == sum(min(t + 1, topk) for n in lens for t in range(n))
    ref = dv.sparse_ref(q, tr.dequantised(pool.cpu()), bt, lens, cu, idx.cpu(), SCALE)
    gs.check(o.cpu(), lse.cpu(), *ref, "the DSA step on the 656-byte and 132-byte rows")
