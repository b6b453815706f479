"""GPU: the attention-sink entries over the bf16 paged KV cache -- cuda_learn_notes_amd.fa2_prefill_paged_varlen_window_sink_bf16 (csrc/
flash_attn_prefill_paged_varlen_window_sink_bf16.cuh) and fa2_decode_paged_multi_window_sink_bf16 (csrc/
flash_attn_decode_paged_multi_window_sink_bf16.cuh) -- against the fp64 reference with the window's mask and one sink logit per query head
(tests/paged_sink_reference.py, which also holds the cases and the sink sets). The criteria are those of tests/test_gpu_paged_window_attention.py,
no new tolerance: O within paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol (per head), -inf LSE entries and
zero rows exactly. Beyond parity: sinks of -inf or -1e30 give the window sibling's bits -- prefill, decode with one split, decode with several --,
a sink changes the result, +1e30 gives exactly 0, a sequence does not depend on its neighbours, two runs repeat their bits, stale table entries
below the window may point at a page of NaN, the rows of no sequence stay untouched, the gpt-oss layer shape, and a captured decode step replays
its bits. Every parity case prints err / bound before it asserts (pytest -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import paged_window_reference as wr  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DS = [64, 128]
FIRST, SPARE = 3, 5
O_FILL, L_FILL = 0x4D2B, 0x4B1DF00D
INT_MAX = sr.INT_MAX
NEG_INF = float("-inf")
bits = lambda t: t.view(torch.int16)  # noqa: E731
fbits = lambda t: t.view(torch.int32)  # noqa: E731


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def run_prefill(q, kp, vp, bt, lens, cu, W, sinks, dev="cuda"):
    """sinks = None: the window sibling (W = None there: a window past the cache)."""
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:2], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    if sinks is None:
        pkg().fa2_prefill_paged_varlen_window_bf16(qd, kd, vd, bd, sl, cd, INT_MAX if W is None else W, o, lse)
    else:
        pkg().fa2_prefill_paged_varlen_window_sink_bf16(qd, kd, vd, bd, sl, cd, W, sinks.to(dev), o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def run_multi(q, kp, vp, bt, lens, W, sinks, dev="cuda"):
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:3], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    if sinks is None:
        pkg().fa2_decode_paged_multi_window_bf16(qd, kd, vd, bd, sl, INT_MAX if W is None else W, o, lse)
    else:
        pkg().fa2_decode_paged_multi_window_sink_bf16(qd, kd, vd, bd, sl, W, sinks.to(dev), o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def check(o, lse, ro, rl, emul, what):
    """O within the emulation bound, LSE within lse_tol head by head, -inf LSE entries and their zero rows exactly. Returns err / bound of O."""
    assert bool(torch.isfinite(o.float()).all()) and not bool(torch.isnan(lse).any()), what
    bo = br.o_bound(emul, ro)
    eo = (o.double() - ro).abs().max().item()
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == NEG_INF).all()), what
    assert bool((o[~fin] == 0).all()), what  # a query that sees no key
    worst = 0.0
    for h in range(rl.shape[-1]):
        f = fin[..., h]
        if bool(f.any()):
            el, bl = (lse[..., h].double()[f] - rl[..., h][f]).abs().max().item(), dr.lse_tol(rl[..., h])
            worst = max(worst, el / bl)
            assert el <= bl, (what, h, el, bl)
    print("%s: O err %.3e / bound %.3e = %.4f   LSE err / bound %.4f" % (what, eo, bo, eo / bo if bo else 0.0, worst))
    assert eo <= bo, (what, eo, bo)
    return eo / bo if bo else 0.0


def nan_page(kp, vp):
    P = kp.shape[0]
    assert bool(torch.isnan(kp[P - 1].float()).all()) and bool(torch.isnan(vp[P - 1].float()).all())
    return P - 1


# ---------------------------------------------------------------------------------------------------- prefill

@pytest.mark.parametrize("page", sr.PREFILL_PAGES)
@pytest.mark.parametrize("heads", sr.PREFILL_HEADS, ids=lambda h: "%dx%d" % h)
@pytest.mark.parametrize("D", DS)
def test_prefill_parity_zero_rows_and_untouched_rows(built, dev, D, heads, page):
    Hq, Hkv = heads
    qs, lens, pool = sr.prefill_case(D, Hq, Hkv, page)
    q, cu = sr.pack(qs, FIRST, SPARE)
    seq = slice(cu[0], cu[-1])
    for W in sr.PREFILL_WINDOWS:
        for name, sinks in (("randn", sr.sinks_randn(Hq, W % 7)), ("mixed", sr.prefill_sinks(Hq, W))):
            o, lse = run_prefill(q, *pool, lens, cu, W, sinks)
            for sl in (slice(0, cu[0]), slice(cu[-1], None)):
                assert bool((bits(o[sl]) == O_FILL).all()) and bool((fbits(lse[sl]) == L_FILL).all()), (D, heads, page, W)
            ro, rl, emul = sr.prefill(q, *pool, lens, cu, W, sinks)
            check(o[seq], lse[seq], ro[seq], rl[seq], emul[seq], "prefill D=%d %dx%d page=%d W=%d %s" % (D, Hq, Hkv, page, W, name))
            dead = slice(cu[4], cu[4] + 2)  # len 2 < T 4: no key, whatever the sink
            assert bool((bits(o[dead]) == 0).all()) and bool((lse[dead] == NEG_INF).all())


@pytest.mark.parametrize("D", DS)
def test_prefill_sinks_of_minus_inf_are_the_window_sibling_bit_for_bit_and_a_packed_sequence_is_its_single_call(built, dev, D):
    for (Hq, Hkv), page in (((8, 1), 16), ((8, 2), 64), ((1, 1), 16)):
        qs, lens, pool = sr.prefill_case(D, Hq, Hkv, page)
        q, cu = sr.pack(qs, FIRST, SPARE)
        for W in sr.PREFILL_WINDOWS:
            o0, l0 = run_prefill(q, *pool, lens, cu, W, None)
            for value in (NEG_INF, -1e30):
                o, lse = run_prefill(q, *pool, lens, cu, W, sr.sinks_const(Hq, value))
                assert torch.equal(bits(o), bits(o0)) and torch.equal(fbits(lse), fbits(l0)), (D, Hq, Hkv, page, W, value)
        o0, l0 = run_prefill(q, *pool, lens, cu, None, None)  # window = None: 2^31 - 1
        o, lse = run_prefill(q, *pool, lens, cu, None, sr.sinks_const(Hq, NEG_INF))
        assert torch.equal(bits(o), bits(o0)) and torch.equal(fbits(lse), fbits(l0))
        # every sequence alone, B = 1, the same sinks: the packed run's bits; and a second packed run repeats them
        sinks = sr.prefill_sinks(Hq, 65)
        o, lse = run_prefill(q, *pool, lens, cu, 65, sinks)
        o2, l2 = run_prefill(q, *pool, lens, cu, 65, sinks)
        assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(l2), fbits(lse))
        kp, vp, bt = pool
        for b, qb in enumerate(qs):
            t = qb.shape[0]
            q1 = torch.cat((qb, torch.full((1,) + tuple(qb.shape[1:]), 2.0 ** 100, dtype=BF)))
            o1, l1 = run_prefill(q1, kp, vp, bt[b:b + 1].contiguous(), [lens[b]], [0, t], 65, sinks)
            assert torch.equal(bits(o1[:t]), bits(o[cu[b]:cu[b + 1]])) and torch.equal(fbits(l1[:t]), fbits(lse[cu[b]:cu[b + 1]])), (D, Hq, b)
            assert bool((bits(o1[t:]) == O_FILL).all())


@pytest.mark.parametrize("D", DS)
def test_prefill_stale_table_entries_below_the_window(built, dev, D):
    Hq, Hkv, page = 8, 2, 16
    qs, lens, (kp, vp, bt) = sr.prefill_case(D, Hq, Hkv, page)
    q, cu = sr.pack(qs, FIRST, SPARE)
    redirected = 0
    for W in (1, 65):
        sinks = sr.prefill_sinks(Hq, W)
        o, lse = run_prefill(q, kp, vp, bt, lens, cu, W, sinks)
        stale, n = wr.stale_table(bt, lens, sr.PREFILL_T, W, page, wr.KEY_STEP, nan_page(kp, vp))
        redirected += n
        o2, l2 = run_prefill(q, kp, vp, stale, lens, cu, W, sinks)
        assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(l2), fbits(lse)), (D, W)
        assert bool(torch.isfinite(o2[cu[0]:cu[-1]].float()).all())
        assert bool((bits(o2[cu[-1]:]) == O_FILL).all()) and bool((bits(o2[:cu[0]]) == O_FILL).all())  # the guard rows
    assert redirected > 0


# ---------------------------------------------------------------------------------------------------- decode

@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("G", sr.DECODE_G)
@pytest.mark.parametrize("T", sr.DECODE_T)
def test_decode_parity_one_split(built, dev, T, G, D):
    Hq, W = sr.ONE_HKV * G, sr.ONE_W
    q, lens, pool = sr.decode_one_case(T, G, D)
    assert pkg().fa2_decode_paged_multi_window_sink_bf16_plan(len(lens), T, Hq, sr.ONE_HKV, sr.ONE_NMAX // sr.PAGE, sr.PAGE, D, W)[0] == 1
    o0, l0 = run_multi(q, *pool, lens, W, None)
    for name, sinks in (("randn", sr.sinks_randn(Hq, T + G)), ("mixed", sr.sinks_mixed(Hq, W))):
        o, lse = run_multi(q, *pool, lens, W, sinks)
        ro, rl, emul = sr.decode(q, *pool, lens, W, sinks)
        check(o, lse, ro, rl, emul, "decode S=1 D=%d T=%d G=%d W=%d %s" % (D, T, G, W, name))
        # a sink does something: len 4096 > W, O moves by more than the bound
        assert float((o[0].double() - o0[0].double()).abs().max()) > br.o_bound(emul, ro), (T, G, D, name)
    for value in (NEG_INF, -1e30):  # ... and none gives the sibling's bits
        o1, l1 = run_multi(q, *pool, lens, W, sr.sinks_const(Hq, value))
        assert torch.equal(bits(o1), bits(o0)) and torch.equal(fbits(l1), fbits(l0)), (T, G, D, value)
    stale, n = wr.stale_table(pool[2], lens, [T] * len(lens), W, sr.PAGE, wr.MULTI_KEY_STEP, nan_page(*pool[:2]))
    assert n > 0
    o2, l2 = run_multi(q, pool[0], pool[1], stale, lens, W, sinks)
    assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(l2), fbits(lse))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("G", sr.DECODE_G)
@pytest.mark.parametrize("T", sr.DECODE_T)
def test_decode_parity_several_splits(built, dev, T, G, D):
    """B = 1, Hkv = 1, max_pages page = 16384: the combine kernel folds the sink. The sink sets are the ones tests/test_paged_sink_surface.py shows
    to be sensitive to a dropped or a double-counted sink."""
    mp = sr.SPLIT_NMAX // sr.PAGE
    for W in sr.SPLIT_WINDOWS:
        assert pkg().fa2_decode_paged_multi_window_sink_bf16_plan(1, T, G, 1, mp, sr.PAGE, D, W)[0] > 1
        for n in sr.DECODE_LENS:
            q, lens, pool = sr.decode_split_case(T, G, D, n)
            sinks = sr.decode_split_sinks(G, n, W)
            o, lse = run_multi(q, *pool, lens, W, sinks)
            ro, rl, emul = sr.decode(q, *pool, lens, W, sinks)
            check(o, lse, ro, rl, emul, "decode S>1 D=%d T=%d G=%d W=%s len=%d" % (D, T, G, W, n))
            o0, l0 = run_multi(q, *pool, lens, W, None)
            for value in (NEG_INF, -1e30):
                o1, l1 = run_multi(q, *pool, lens, W, sr.sinks_const(G, value))
                assert torch.equal(bits(o1), bits(o0)) and torch.equal(fbits(l1), fbits(l0)), (T, G, D, W, n, value)
            o2, l2 = run_multi(q, *pool, lens, W, sinks)  # two runs repeat their bits
            assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(l2), fbits(lse))


@pytest.mark.parametrize("D", DS)
def test_huge_sinks_give_exact_zeros_and_large_ones_small_finite_rows(built, dev, D):
    """+1e30: O exactly 0 and LSE the sink, no NaN or inf anywhere but the -inf of the rows without a key; +30: finite O near 0, within the bound."""
    T, G = 3, 4
    cases = [(run_multi, sr.decode, sr.decode_one_case(T, G, D), sr.ONE_HKV * G, (sr.ONE_W,)),
             (run_multi, sr.decode, sr.decode_split_case(T, G, D, 4096), G, (1000,))]
    qs, plens, ppool = sr.prefill_case(D, 8, 2, 16)
    pq, cu = sr.pack(qs)
    for value in (1e30, 30.0):
        outs = []
        for run, ref, (q, lens, pool), Hq, args in cases:
            sinks = sr.sinks_const(Hq, value)
            o, lse = run(q, *pool, lens, *args, sinks)
            outs.append((o, lse, ref(q, *pool, lens, *args, sinks)))
        sinks = sr.sinks_const(8, value)
        o, lse = run_prefill(pq, *ppool, plens, cu, 65, sinks)
        outs.append((o, lse, sr.prefill(pq, *ppool, plens, cu, 65, sinks)))
        for i, (o, lse, (ro, rl, emul)) in enumerate(outs):
            check(o, lse, ro, rl, emul, "sink %g D=%d case %d" % (value, D, i))
            live = torch.isfinite(rl)
            assert not bool(torch.isnan(lse).any()) and not bool(torch.isnan(o.float()).any()) and not bool((lse == float("inf")).any())
            if value == 1e30:
                assert bool((o == 0).all()) and bool(((lse[live] / 1e30 - 1).abs() < 1e-6).all())
            else:
                assert float(o.float().abs().max()) < 1e-6 and float(o.float().abs().max()) > 0 and bool(((lse[live] - 30).abs() < 1e-3).all())


# ---------------------------------------------------------------------------------------------------- the gpt-oss layer shape

def test_gpt_oss_layer_pair_prefill_then_decode(built, dev):
    """Hq 64, Hkv 8, D 64, page 16: a prefill over [130, 7] tokens at W = 128 (the sliding layers) and W = None (the full layers), then one T = 1
    decode step on the same cache."""
    Hq, Hkv, D, page, Nmax = 64, 8, 64, 16, 256
    g = torch.Generator().manual_seed(64)
    k, v = (torch.randn(2, Hkv, Nmax, D, generator=g).to(BF) for _ in range(2))
    sinks = sr.sinks_randn(Hq, 64) + 2.0  # learned sinks of the size of the rows' log-sum-exp
    Ts, lens = [130, 7], [130, 7]
    qs = tuple(torch.randn(t, Hq, D, generator=g).to(BF) for t in Ts)
    q, cu = sr.pack(qs)
    step_lens = [131, 8]
    pool = pr.make_pool(k, v, page, step_lens, seed=1)  # the cache holds the step's token too; the prefill does not see it
    qd = torch.randn(2, 1, Hq, D, generator=g).to(BF)
    for W in (128, None):
        o, lse = run_prefill(q, *pool, lens, cu, W, sinks)
        check(o, lse, *sr.prefill(q, *pool, lens, cu, W, sinks), "gpt-oss prefill W=%s" % W)
        o, lse = run_multi(qd, *pool, step_lens, W, sinks)
        check(o, lse, *sr.decode(qd, *pool, step_lens, W, sinks), "gpt-oss decode W=%s" % W)


# ---------------------------------------------------------------------------------------------------- captured replay

def test_captured_decode_step_replays_the_eager_bits(built, dev):
    """One decode step captured into a graph on a single stream; the replay on changed q, lengths and sinks equals the eager call's bits."""
    T, G, D = 1, 8, 64
    Hq = sr.ONE_HKV * G
    q, lens, pool = sr.decode_one_case(T, G, D)
    qd, kd, vd, bd = (t.to(dev) for t in (q, *pool))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    sk = sr.sinks_randn(Hq, 1).to(dev)
    og, lg = torch.empty_like(qd), torch.empty(qd.shape[:3], dtype=torch.float32, device=dev)

    def step(o, lse):
        pkg().fa2_decode_paged_multi_window_sink_bf16(qd, kd, vd, bd, sl, sr.ONE_W, sk, o, lse)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(og, lg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(og, lg)
    for i in range(2):
        gen = torch.Generator().manual_seed(i)
        qd.copy_(torch.randn(q.shape, generator=gen).to(BF)), sk.copy_(sr.sinks_mixed(Hq, sr.ONE_W + i))
        sl.copy_(torch.tensor([max(n - 7 * (i + 1), 0) for n in lens], dtype=torch.int32))  # shorter: the table's live entries cover them
        og.fill_(float("nan")), lg.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        oe, le = torch.full_like(og, float("nan")), torch.full_like(lg, float("nan"))
        step(oe, le)
        torch.cuda.synchronize()
        assert torch.equal(bits(og.cpu()), bits(oe.cpu())) and torch.equal(fbits(lg.cpu()), fbits(le.cpu())), i
        assert not bool(torch.isnan(og.float()).any())
