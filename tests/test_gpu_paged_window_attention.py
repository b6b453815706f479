"""GPU: the sliding-window attention entries over the bf16 paged KV cache -- cuda_learn_notes_amd.fa2_prefill_paged_varlen_window_bf16 (csrc/
flash_attn_prefill_paged_varlen_window_bf16.cuh) and fa2_decode_paged_multi_window_bf16 (csrc/flash_attn_decode_paged_multi_window_bf16.cuh) --
against the fp64 reference over the gathered dense cache with the window's mask (tests/paged_window_reference.py). The criteria are those of
tests/test_gpu_paged_bf16_attention.py: O within paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol, -inf LSE
entries and zero rows exactly. Beyond parity: a window past the cache gives the unwindowed entries' bits, a window inside it does not give their
result, a sequence does not depend on its neighbours, two runs repeat their bits, the rows of no sequence stay untouched, and table entries of
pages wholly below the window may point anywhere (here: at a valid page of NaN). Pools come from paged_decode_reference.make_pool. A run and its
references are computed once and shared by the tests that look at them. Every parity case prints err / bound before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import paged_window_reference as wr  # noqa: E402
import prefill_varlen_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DS = [64, 128]
# (Hkv, G, page, max_pages), T_b: G in {1, 4, 8}, pages 16 and 256, T_b in {0, 1, 129, 130}; max_pages page >= 700 + 130
CASES = [((2, 1, 16, 52), [129, 0, 1, 130]), ((1, 4, 256, 4), [130, 1, 0, 129]), ((1, 8, 16, 52), [1, 129, 130, 0])]
CASE_IDS = ["x".join(map(str, g)) for g, _ in CASES]
CONTEXTS = [0, 63, 64, 200, 700]  # keys in front of the new tokens
# the window's edge inside the first step (1, 17), on a step boundary (64), one past it (65), inside a tile's row range (17 < 128 / G tokens),
# and with 700 keys in front a first step k_begin > 0 for every tile (200)
WINDOWS = [1, 17, 64, 65, 200]
FIRST, SPARE = 3, 5
O_FILL, L_FILL = 0x4D2B, 0x4B1DF00D
PAST = wr.INT_MAX  # a window past any cache
bits = lambda t: t.view(torch.int16)  # noqa: E731
fbits = lambda t: t.view(torch.int32)  # noqa: E731


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


@functools.lru_cache(maxsize=None)
def problem(ci, D):
    """Gaussian bf16 (q_b [T_b,Hq,D] per sequence, dense k, v [B,Hkv,Nmax,D]) on the CPU, made once and never modified."""
    (Hkv, G, page, mp), T = CASES[ci]
    g = torch.Generator().manual_seed(131 * ci + D)
    qs = tuple(torch.randn(t, Hkv * G, D, generator=g).to(BF) for t in T)
    k, v = (torch.randn(len(T), Hkv, page * mp, D, generator=g).to(BF) for _ in range(2))
    return qs, k, v


def pack(qs, first=FIRST, spare=SPARE):
    """(q [total_q,Hq,D], cu): the sequences packed from row `first` on; the rows of no sequence hold 2^100."""
    cu = vr.cu_of([x.shape[0] for x in qs], first)
    q = torch.full((cu[-1] + spare,) + tuple(qs[0].shape[1:]), 2.0 ** 100, dtype=BF)
    for b, x in enumerate(qs):
        q[cu[b]:cu[b + 1]] = x
    return q, cu


def run_prefill(q, kp, vp, bt, lens, cu, W, dev="cuda"):
    """W = None: the unwindowed sibling."""
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:2], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    if W is None:
        pkg().fa2_prefill_paged_varlen_bf16(qd, kd, vd, bd, sl, cd, o, lse)
    else:
        pkg().fa2_prefill_paged_varlen_window_bf16(qd, kd, vd, bd, sl, cd, W, o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def check(o, lse, ro, rl, emul, what):
    """O within the emulation bound, LSE within lse_tol, -inf LSE entries and their zero rows exactly. Returns err / bound of O."""
    assert bool(torch.isfinite(o).all()), what
    bo = br.o_bound(emul, ro)
    eo = (o.double() - ro).abs().max().item()
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float("-inf")).all()), what
    assert bool((o[~fin] == 0).all()), what  # a query that sees no key
    el = (lse.double()[fin] - rl[fin]).abs().max().item() if bool(fin.any()) else 0.0
    bl = dr.lse_tol(rl)
    print("%s: O err %.3e / bound %.3e = %.4f   LSE err %.3e / bound %.3e = %.4f" % (what, eo, bo, eo / bo, el, bl, el / bl))
    assert eo <= bo, (what, eo, bo)
    assert el <= bl, (what, el, bl)
    return eo / bo


@functools.lru_cache(maxsize=None)
def pool_of(ci, D, ctx):
    (Hkv, G, page, mp), T = CASES[ci]
    qs, k, v = problem(ci, D)
    q, cu = pack(qs)
    lens = [min(ctx, page * mp - t) + t for t in T]
    return q, cu, lens, pr.make_pool(k, v, page, lens, seed=ctx)


@functools.lru_cache(maxsize=None)
def packed_run(ci, D, ctx, W):
    """One packed windowed call with `ctx` keys in front of every sequence's new tokens (W = None: the unwindowed sibling)."""
    q, cu, lens, pool = pool_of(ci, D, ctx)
    return run_prefill(q, *pool, lens, cu, W)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_prefill_parity_and_untouched_rows(built, dev, ci, D):
    for ctx in CONTEXTS:
        q, cu, lens, pool = pool_of(ci, D, ctx)
        seq = slice(cu[0], cu[-1])
        for W in WINDOWS:
            o, lse = packed_run(ci, D, ctx, W)
            for sl in (slice(0, cu[0]), slice(cu[-1], None)):
                assert bool((bits(o[sl]) == O_FILL).all()) and bool((fbits(lse[sl]) == L_FILL).all()), (ci, D, ctx, W)
            ro, rl, emul = wr.prefill(q, *pool, lens, cu, W)
            check(o[seq], lse[seq], ro[seq], rl[seq], emul[seq], "prefill D=%d %s ctx=%d W=%d lens=%s" % (D, CASE_IDS[ci], ctx, W, lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_prefill_window_past_the_cache_is_the_unwindowed_entry_bit_for_bit_and_a_window_inside_is_not(built, dev, ci, D):
    (Hkv, G, page, mp), T = CASES[ci]
    for ctx in CONTEXTS:
        o0, l0 = packed_run(ci, D, ctx, None)
        for W in (page * mp, PAST):
            o, lse = packed_run(ci, D, ctx, W)
            assert torch.equal(bits(o), bits(o0)) and torch.equal(fbits(lse), fbits(l0)), (ci, D, ctx, W)
    q, cu, lens, _ = pool_of(ci, D, 700)
    assert max(lens) > 200
    for W in WINDOWS:  # len > W: another function, another result
        o, lse = packed_run(ci, D, 700, W)
        o0, l0 = packed_run(ci, D, 700, None)
        seq = slice(cu[0], cu[-1])
        assert float((o[seq].float() - o0[seq].float()).abs().max()) > 0.05 and not torch.equal(fbits(lse[seq]), fbits(l0[seq])), (ci, D, W)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_prefill_sequence_does_not_depend_on_its_neighbours(built, dev, ci, D):
    """Every sequence of the packed runs, called alone with B = 1 and the same window: the same bits, O and LSE."""
    qs = problem(ci, D)[0]
    for ctx in (63, 700):
        q, cu, lens, (kp, vp, bt) = pool_of(ci, D, ctx)
        for W in WINDOWS:
            o, lse = packed_run(ci, D, ctx, W)
            for b, qb in enumerate(qs):
                t = qb.shape[0]
                q1 = torch.cat((qb, torch.full((1,) + tuple(qb.shape[1:]), 2.0 ** 100, dtype=BF)))  # one spare row: total_q >= 1 also for T_b = 0
                o1, l1 = run_prefill(q1, kp, vp, bt[b:b + 1].contiguous(), [lens[b]], [0, t], W)
                assert torch.equal(bits(o1[:t]), bits(o[cu[b]:cu[b + 1]])) and torch.equal(fbits(l1[:t]), fbits(lse[cu[b]:cu[b + 1]])), (ci, D, ctx, W, b)
                assert bool((bits(o1[t:]) == O_FILL).all())


def nan_page(kp, vp):
    """The index of a VALID pool page that holds NaN in both pools: make_pool's poison page, the last one."""
    P = kp.shape[0]
    assert bool(torch.isnan(kp[P - 1].float()).all()) and bool(torch.isnan(vp[P - 1].float()).all())
    return P - 1


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_prefill_reads_no_table_entry_of_a_page_below_the_window(built, dev, ci, D):
    """Every table entry of a page that ends at or before align_down(max(0, len_b - T_b - W + 1), max(page, 64)) redirected to a page of NaN: the
    bits of the run with the true table, and finite. Also: two runs repeat their bits."""
    (Hkv, G, page, mp), T = CASES[ci]
    redirected = 0
    for ctx in (200, 700):
        q, cu, lens, (kp, vp, bt) = pool_of(ci, D, ctx)
        for W in WINDOWS:
            o, lse = packed_run(ci, D, ctx, W)
            stale, n = wr.stale_table(bt, lens, T, W, page, wr.KEY_STEP, nan_page(kp, vp))
            redirected += n
            o2, l2 = run_prefill(q, kp, vp, stale, lens, cu, W)
            assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(l2), fbits(lse)), (ci, D, ctx, W)
            assert bool(torch.isfinite(o2[cu[0]:cu[-1]].float()).all())
    assert redirected > 0
    o, lse = packed_run(ci, D, 700, 65)
    q, cu, lens, pool = pool_of(ci, D, 700)
    o2, l2 = run_prefill(q, *pool, lens, cu, 65)
    assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(l2), fbits(lse))


# ---------------------------------------------------------------------------------------------------- multi-token decode

PAGE = 16
MULTI_WINDOWS = [1, 33, 128, 129, 1000]


def multi_lens(W, T, Nmax):
    return [min(n, Nmax) for n in (0, 1, W - 1, W, W + T - 1, 5 * W + 3, Nmax)]


@functools.lru_cache(maxsize=None)
def multi_problem(B, T, Hkv, G, Nmax, D):
    g = torch.Generator().manual_seed(1000 * T + 10 * G + D + B + Nmax)
    q = torch.randn(B, T, Hkv * G, D, generator=g).to(BF)
    k, v = (torch.randn(B, Hkv, Nmax, D, generator=g).to(BF) for _ in range(2))
    return q, k, v


def run_multi(q, kp, vp, bt, lens, W, exact_workspace=False, dev="cuda"):
    """The call on copies (W = None: the unwindowed sibling); with exact_workspace a caller's workspace of exactly the planned bytes in front of a
    guard band that must stay intact."""
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:3], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    ws = None
    if exact_workspace:
        B, T, Hq, D = q.shape
        need = pkg().fa2_decode_paged_multi_window_bf16_plan(B, T, Hq, kp.shape[1], bt.shape[1], kp.shape[2], D, W)[2]
        assert need > 0
        buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        ws = buf[:need]
    if W is None:
        pkg().fa2_decode_paged_multi_bf16(qd, kd, vd, bd, sl, o, lse)
    else:
        pkg().fa2_decode_paged_multi_window_bf16(qd, kd, vd, bd, sl, W, o, lse, ws)
    torch.cuda.synchronize()
    if exact_workspace:
        assert bool((buf[need:] == 0xA5).all()), "the guard band behind the workspace"
    return o.cpu(), lse.cpu()


def multi_case(q, k, v, lens, W, what, exact_workspace=False):
    """Parity of one call; then the stale table of this W: the same bits, finite."""
    T = q.shape[1]
    kp, vp, bt = pr.make_pool(k, v, PAGE, lens, seed=W % 97)
    o, lse = run_multi(q, kp, vp, bt, lens, W, exact_workspace)
    ro, rl, emul = wr.decode(q, kp, vp, bt, lens, W)
    check(o, lse, ro, rl, emul, what)
    stale, n = wr.stale_table(bt, lens, [T] * len(lens), W, PAGE, wr.MULTI_KEY_STEP, nan_page(kp, vp))
    o2, l2 = run_multi(q, kp, vp, stale, lens, W)  # the wrapper's own workspace, and a second run
    assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(l2), fbits(lse)), what
    return o, lse, (kp, vp, bt), n


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("T", [1, 4, 8])
def test_multi_parity_one_split(built, dev, T, G, D):
    """max_pages page = 304: one split whatever W is. Lengths 0, 1, W - 1, W, W + T - 1, 5 W + 3 and Nmax, each clipped to Nmax."""
    Hkv, Nmax = 2, 304
    redirected = 0
    for W in MULTI_WINDOWS:
        lens = multi_lens(W, T, Nmax)
        assert pkg().fa2_decode_paged_multi_window_bf16_plan(len(lens), T, Hkv * G, Hkv, Nmax // PAGE, PAGE, D, W)[0] == 1
        q, k, v = multi_problem(len(lens), T, Hkv, G, Nmax, D)
        o, lse, pool, n = multi_case(q, k, v, lens, W, "multi D=%d T=%d G=%d W=%d lens=%s" % (D, T, G, W, lens))
        redirected += n
        if W < Nmax - T:  # the full sequence sees more than W keys without the window
            o0, _ = run_multi(q, *pool, lens, None)
            assert float((o[-1].float() - o0[-1].float()).abs().max()) > 0.05, (T, G, D, W)
    assert redirected > 0
    o0, l0 = run_multi(q, *pool, lens, None)
    for W in (Nmax, PAST):  # a window past the cache: the unwindowed entry's bits
        o, lse = run_multi(q, *pool, lens, W)
        assert torch.equal(bits(o), bits(o0)) and torch.equal(fbits(lse), fbits(l0)), (T, G, D, W)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("T,G", [(1, 1), (4, 4), (8, 8)])
def test_multi_parity_split_over_the_window_with_a_callers_workspace(built, dev, T, G, D):
    """max_pages page = 4096 with one KV head and W = 1000: 3 splits of 384 keys counted from each sequence's base. Lengths that put the base at 0
    (below W + T), on a multiple of 128 with every split live (4096, 2500), and 0; the workspace is the caller's, exactly the planned bytes."""
    Hkv, Nmax, W = 1, 4096, 1000
    lens = multi_lens(W, T, Nmax) + [2500, 1151 + T, 500]
    S, C, ws = pkg().fa2_decode_paged_multi_window_bf16_plan(len(lens), T, Hkv * G, Hkv, Nmax // PAGE, PAGE, D, W)
    assert (S, C) == (3, 384) and ws == len(lens) * T * Hkv * G * S * (D + 2) * 4
    assert {wr.live_splits(n, T, W, PAGE, C) for n in lens} == {0, 1, 2, 3}
    q, k, v = multi_problem(len(lens), T, Hkv, G, Nmax, D)
    o, lse, pool, n = multi_case(q, k, v, lens, W, "multi split D=%d T=%d G=%d lens=%s" % (D, T, G, lens), exact_workspace=True)
    assert n > 100  # 4096 keys with a window of 1000: most pages are below it
    o0, l0 = run_multi(q, *pool, lens, None)
    full = lens.index(Nmax)
    assert float((o[full].float() - o0[full].float()).abs().max()) > 0.02  # len 4096 > W
    for Wp in (Nmax, PAST):  # a window past the cache: the unwindowed plan (16 splits) and the unwindowed entry's bits
        assert pkg().fa2_decode_paged_multi_window_bf16_plan(len(lens), T, Hkv * G, Hkv, Nmax // PAGE, PAGE, D, Wp)[:2] == (16, 256)
        o1, l1 = run_multi(q, *pool, lens, Wp, exact_workspace=True)
        assert torch.equal(bits(o1), bits(o0)) and torch.equal(fbits(l1), fbits(l0)), (T, G, D, Wp)
