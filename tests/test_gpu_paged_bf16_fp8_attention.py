"""GPU: the bf16 paged attention entries over FP8 (e4m3) pools -- cuda_learn_notes_amd.fa2_prefill_paged_varlen_window_sink_bf16_fp8 (csrc/
flash_attn_prefill_paged_varlen_window_sink_bf16_fp8.cuh) and fa2_decode_paged_multi_window_sink_bf16_fp8 (csrc/
flash_attn_decode_paged_multi_window_sink_bf16_fp8.cuh) -- against the fp64 reference and the bf16 emulation of paged_sink_reference ON THE
DEQUANTISED POOLS (tests/paged_bf16_fp8_reference.py, which holds the cases and the scales). No new tolerance: O within
paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol per head, -inf LSE entries and zero rows exactly. Every parity
case runs with per-head scales that tests/test_paged_bf16_fp8_surface.py shows to be sensitive to a dropped or a neighbour's scale. Beyond parity,
bit for bit: a packed sequence is its B = 1 call, two runs repeat, sinks = None is a tensor of -inf is -1e30, +1e30 gives O = 0 and LSE = the
sink, window = None is any W >= Nmax, doubling v_scale of one KV head doubles exactly its heads' O, stale table entries may point at a page of
0x7F bytes, the captured append -> decode pair replays the eager bits; all 254 finite codes convert exactly. Every parity case prints err / bound
before it asserts (pytest -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import fp8_paged_attn_cases as cs  # noqa: E402
import paged_bf16_fp8_reference as fr  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import paged_window_reference as wr  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DS = [64, 128]
FIRST, SPARE = 3, 5
O_FILL, L_FILL = sk.O_FILL, sk.L_FILL
NEG_INF = float("-inf")
bits, fbits, check = sk.bits, sk.fbits, sk.check
RATIOS = {}  # the largest err / bound per kernel family, printed by the last test of the file


def note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def run_prefill(q, pool, lens, cu, ks, vs, W, sinks, dev="cuda"):
    qd, kd, vd, bd, ksd, vsd = (t.to(dev) for t in (q, *pool, ks, vs))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:2], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    pkg().fa2_prefill_paged_varlen_window_sink_bf16_fp8(qd, kd, vd, bd, sl, cd, ksd, vsd, W, None if sinks is None else sinks.to(dev), o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def run_multi(q, pool, lens, ks, vs, W, sinks, dev="cuda"):
    qd, kd, vd, bd, ksd, vsd = (t.to(dev) for t in (q, *pool, ks, vs))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:3], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    pkg().fa2_decode_paged_multi_window_sink_bf16_fp8(qd, kd, vd, bd, sl, ksd, vsd, W, None if sinks is None else sinks.to(dev), o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def huge_sink_lse(value=1e30):
    """LSE of a row under a sink that far above its scores, to the bit: the kernels form sink2 = fl(sink log2 e), the row's l becomes
    fma(l, exp2(m - sink2) = 0, exp2(0) = 1) = 1, and LSE = fl((sink2 + log2 1) ln 2) -- two fp32 products of the fp32 sink."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    return float((f(value) * f(1.4426950408889634)) * f(0.6931471805599453))


def same(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(fbits(a[1]), fbits(b[1]))


def nan_page(pool):
    """The pool's last page: no live entry names it and it holds 0x7F in K and V, as every other page no live entry names."""
    kp, vp, bt = pool
    P = kp.shape[0]
    assert bool((f8.bits(kp[P - 1]) == fr.NAN_BYTE).all()) and bool((f8.bits(vp[P - 1]) == fr.NAN_BYTE).all())
    return P - 1


# ---------------------------------------------------------------------------------------------------- prefill

@pytest.mark.parametrize("page", sr.PREFILL_PAGES)
@pytest.mark.parametrize("heads", sr.PREFILL_HEADS, ids=lambda h: "%dx%d" % h)
@pytest.mark.parametrize("D", DS)
def test_prefill_parity_zero_rows_and_untouched_rows(built, dev, D, heads, page):
    Hq, Hkv = heads
    qs, lens, pool, ks, vs = fr.prefill_case(D, Hq, Hkv, page)
    nan_page(pool)
    q, cu = sr.pack(qs, FIRST, SPARE)
    seq = slice(cu[0], cu[-1])
    for W in fr.PREFILL_WINDOWS:
        for name, sinks in (("mixed", sr.prefill_sinks(Hq, sr.INT_MAX if W is None else W)), ("none", None)):
            o, lse = run_prefill(q, pool, lens, cu, ks, vs, W, sinks)
            for sl in (slice(0, cu[0]), slice(cu[-1], None)):
                assert bool((bits(o[sl]) == O_FILL).all()) and bool((fbits(lse[sl]) == L_FILL).all()), (D, heads, page, W)
            ro, rl, emul = fr.prefill(q, *pool, lens, cu, ks, vs, W, sinks)
            note("prefill", check(o[seq], lse[seq], ro[seq], rl[seq], emul[seq],
                                  "fp8 prefill D=%d %dx%d page=%d W=%s %s" % (D, Hq, Hkv, page, W, name)))
            dead = slice(cu[4], cu[4] + 2)  # len 2 < T 4: no key, whatever the sink
            assert bool((bits(o[dead]) == 0).all()) and bool((lse[dead] == NEG_INF).all())


@pytest.mark.parametrize("D", DS)
def test_prefill_exact_properties(built, dev, D):
    for (Hq, Hkv), page in (((8, 2), 16), ((1, 1), 64)):
        qs, lens, pool, ks, vs = fr.prefill_case(D, Hq, Hkv, page)
        q, cu = sr.pack(qs, FIRST, SPARE)
        seq = slice(cu[0], cu[-1])
        for W in (65, None):
            none = run_prefill(q, pool, lens, cu, ks, vs, W, None)
            for value in (NEG_INF, -1e30):  # sinks = None is a tensor of -inf, and a sink that far below every row changes no bit
                assert same(run_prefill(q, pool, lens, cu, ks, vs, W, sr.sinks_const(Hq, value)), none), (D, Hq, W, value)
            o, lse = run_prefill(q, pool, lens, cu, ks, vs, W, sr.sinks_const(Hq, 1e30))
            live = torch.isfinite(none[1][seq])
            assert bool((o[seq] == 0).all()) and bool((lse[seq][live] == huge_sink_lse()).all()) and bool((lse[seq][~live] == NEG_INF).all())
        full = run_prefill(q, pool, lens, cu, ks, vs, None, None)  # window = None: any W >= Nmax
        for W in (sr.PREFILL_NMAX, sr.PREFILL_NMAX + 77):
            assert same(run_prefill(q, pool, lens, cu, ks, vs, W, None), full), (D, Hq, W)
        sinks = sr.prefill_sinks(Hq, 65)
        packed = run_prefill(q, pool, lens, cu, ks, vs, 65, sinks)
        assert same(run_prefill(q, pool, lens, cu, ks, vs, 65, sinks), packed)  # two runs repeat their bits
        kp, vp, bt = pool
        for b, qb in enumerate(qs):  # every sequence alone, B = 1: the packed run's bits
            t = qb.shape[0]
            q1 = torch.cat((qb, torch.full((1,) + tuple(qb.shape[1:]), 2.0 ** 100, dtype=BF)))
            o1, l1 = run_prefill(q1, (kp, vp, bt[b:b + 1].contiguous()), [lens[b]], [0, t], ks, vs, 65, sinks)
            assert torch.equal(bits(o1[:t]), bits(packed[0][cu[b]:cu[b + 1]])) and torch.equal(fbits(l1[:t]), fbits(packed[1][cu[b]:cu[b + 1]]))
            assert bool((bits(o1[t:]) == O_FILL).all())


@pytest.mark.parametrize("D", DS)
def test_doubling_v_scale_of_one_head_doubles_exactly_its_rows(built, dev, D):
    """Prefill (8 x 2 heads), decode with one split (Hkv 8) and with several (Hkv 1): O of the query heads of the doubled KV head doubles bit for
    bit (a bf16 exponent step; |O| stays far from overflow and from the subnormals' precision loss: asserted), LSE and every other head keep
    their bits."""
    def doubled(run, Hkv, G, kvh):
        ks, vs = fr.scales(Hkv)
        v2 = vs.clone()
        v2[kvh] *= 2
        (o, lse), (o2, l2) = run(vs), run(v2)
        assert torch.equal(fbits(lse), fbits(l2))
        mine = torch.zeros(Hkv * G, dtype=torch.bool)
        mine[kvh * G:(kvh + 1) * G] = True
        a = o[..., mine, :].float()
        assert float(a.abs().max()) < 1e30 and float(a[a != 0].abs().min()) > 1e-30
        assert torch.equal(bits((a * 2).to(BF)), bits(o2[..., mine, :])) and torch.equal(bits(o[..., ~mine, :]), bits(o2[..., ~mine, :]))

    qs, lens, pool, ks, _ = fr.prefill_case(D, 8, 2, 16)
    q, cu = sr.pack(qs)
    doubled(lambda vs: run_prefill(q, pool, lens, cu, ks, vs, 65, sr.prefill_sinks(8, 65)), 2, 4, 1)
    q, lens, pool, ks, _ = fr.decode_one_case(3, 4, D)
    doubled(lambda vs: run_multi(q, pool, lens, ks, vs, sr.ONE_W, sr.sinks_mixed(32, sr.ONE_W)), sr.ONE_HKV, 4, 5)
    q, lens, pool, ks, _ = fr.decode_split_case(8, D, 4096)
    doubled(lambda vs: run_multi(q, pool, lens, ks, vs, 1000, sr.decode_split_sinks(8, 4096, 1000)), 1, 8, 0)


@pytest.mark.parametrize("D", DS)
def test_prefill_stale_table_entries_point_at_a_page_of_nan_bytes(built, dev, D):
    Hq, Hkv, page = 8, 2, 16
    qs, lens, pool, ks, vs = fr.prefill_case(D, Hq, Hkv, page)
    q, cu = sr.pack(qs, FIRST, SPARE)
    redirected = 0
    for W in (1, 65):
        sinks = sr.prefill_sinks(Hq, W)
        good = run_prefill(q, pool, lens, cu, ks, vs, W, sinks)
        stale, n = wr.stale_table(pool[2], lens, sr.PREFILL_T, W, page, wr.KEY_STEP, nan_page(pool))
        redirected += n
        got = run_prefill(q, (pool[0], pool[1], stale), lens, cu, ks, vs, W, sinks)
        assert same(got, good), (D, W)
        assert bool(torch.isfinite(got[0][cu[0]:cu[-1]].float()).all())
    assert redirected > 0


# ---------------------------------------------------------------------------------------------------- decode

@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("G", sr.DECODE_G)
@pytest.mark.parametrize("T", sr.DECODE_T)
def test_decode_parity_one_split(built, dev, T, G, D):
    Hq, W = sr.ONE_HKV * G, sr.ONE_W
    q, lens, pool, ks, vs = fr.decode_one_case(T, G, D)
    nan_page(pool)
    assert pkg().fa2_decode_paged_multi_window_sink_bf16_fp8_plan(len(lens), T, Hq, sr.ONE_HKV, sr.ONE_NMAX // sr.PAGE, sr.PAGE, D, W)[0] == 1
    sinks = sr.sinks_mixed(Hq, W)
    got = run_multi(q, pool, lens, ks, vs, W, sinks)
    note("decode, one split", check(*got, *fr.decode(q, *pool, lens, ks, vs, W, sinks), "fp8 decode S=1 D=%d T=%d G=%d W=%d mixed" % (D, T, G, W)))
    assert same(run_multi(q, pool, lens, ks, vs, W, sinks), got)  # two runs repeat their bits
    none = run_multi(q, pool, lens, ks, vs, W, None)
    note("decode, one split", check(*none, *fr.decode(q, *pool, lens, ks, vs, W, None), "fp8 decode S=1 D=%d T=%d G=%d W=%d none" % (D, T, G, W)))
    for value in (NEG_INF, -1e30):
        assert same(run_multi(q, pool, lens, ks, vs, W, sr.sinks_const(Hq, value)), none), (T, G, D, value)
    o, lse = run_multi(q, pool, lens, ks, vs, W, sr.sinks_const(Hq, 1e30))  # +1e30: O exactly 0, LSE the sink to the bit
    live = torch.isfinite(none[1])
    assert bool((o == 0).all()) and bool((lse[live] == huge_sink_lse()).all()) and bool((lse[~live] == NEG_INF).all()) and bool(live.any())
    stale, n = wr.stale_table(pool[2], lens, [T] * len(lens), W, sr.PAGE, wr.MULTI_KEY_STEP, nan_page(pool))
    assert n > 0
    again = run_multi(q, (pool[0], pool[1], stale), lens, ks, vs, W, sinks)
    assert same(again, got) and bool(torch.isfinite(again[0].float()).all())


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("G", fr.SPLIT_G)
def test_decode_parity_several_splits(built, dev, G, D):
    """B = 1, Hkv = 1, T = 1, max_pages page = 16384: the splits hand over partials that carry v_scale, the siblings' combine kernels merge them
    (with sinks the sink one, without the window one)."""
    mp = sr.SPLIT_NMAX // sr.PAGE
    for W in sr.SPLIT_WINDOWS:
        assert pkg().fa2_decode_paged_multi_window_sink_bf16_fp8_plan(1, 1, G, 1, mp, sr.PAGE, D, W)[0] > 1
        for n in fr.SPLIT_LENS:
            q, lens, pool, ks, vs = fr.decode_split_case(G, D, n)
            sinks = sr.decode_split_sinks(G, n, W)
            got = run_multi(q, pool, lens, ks, vs, W, sinks)
            note("decode, several splits",
                 check(*got, *fr.decode(q, *pool, lens, ks, vs, W, sinks), "fp8 decode S>1 D=%d G=%d W=%s len=%d mixed" % (D, G, W, n)))
            assert same(run_multi(q, pool, lens, ks, vs, W, sinks), got)
            none = run_multi(q, pool, lens, ks, vs, W, None)
            note("decode, several splits",
                 check(*none, *fr.decode(q, *pool, lens, ks, vs, W, None), "fp8 decode S>1 D=%d G=%d W=%s len=%d none" % (D, G, W, n)))
            for value in (NEG_INF, -1e30):
                assert same(run_multi(q, pool, lens, ks, vs, W, sr.sinks_const(G, value)), none), (G, D, W, n, value)
            o, lse = run_multi(q, pool, lens, ks, vs, W, sr.sinks_const(G, 1e30))
            assert bool((o == 0).all()) and bool((lse == huge_sink_lse()).all())
        q, lens, pool, ks, vs = fr.decode_split_case(G, D, 4096)
    full = run_multi(q, pool, lens, ks, vs, None, None)  # window = None: any W >= Nmax
    assert same(run_multi(q, pool, lens, ks, vs, sr.SPLIT_NMAX, None), full)
    stale, n = wr.stale_table(pool[2], lens, [1], 1000, sr.PAGE, wr.MULTI_KEY_STEP, nan_page(pool))
    assert n > 0
    sinks = sr.decode_split_sinks(G, 4096, 1000)
    assert same(run_multi(q, (pool[0], pool[1], stale), lens, ks, vs, 1000, sinks), run_multi(q, pool, lens, ks, vs, 1000, sinks))


# ---------------------------------------------------------------------------------------------------- every code, on the hardware

@pytest.mark.parametrize("D", DS)
def test_all_finite_codes_against_the_fp64_reference(built, dev, D):
    """K and V rows that run through all 254 finite e4m3 codes, subnormals included, scale 1: prefill (70 tokens x 2 heads: a full row tile and a
    partly empty one) and decode (one split, and T = 3 x G = 4) against the fp64 reference on the dequantised pool."""
    k8, v8, ks, vs, N = fr.all_codes_case(D)
    g = torch.Generator().manual_seed(D)
    n = 300
    pool = f8.make_pool(k8, v8, 16, [n], seed=3)
    q = (torch.randn(70, 2, D, generator=g) / 64).to(BF)
    got = run_prefill(q, pool, [n], [0, 70], ks, vs, None, None)
    note("all codes", check(*got, *fr.prefill(q, *pool, [n], [0, 70], ks, vs, None, None), "all codes prefill D=%d" % D))
    q = (torch.randn(1, 3, 4, D, generator=g) / 64).to(BF)
    for W in (None, 100):
        got = run_multi(q, pool, [n], ks, vs, W, None)
        note("all codes", check(*got, *fr.decode(q, *pool, [n], ks, vs, W, None), "all codes decode D=%d W=%s" % (D, W)))


@pytest.mark.parametrize("D", DS)
def test_every_value_code_comes_out_bit_for_bit(built, dev, D):
    """fp8_paged_attn_cases.all_codes_problem (one-hot keys under k_scale 1/2, V rows that cycle through the 254 finite bytes under v_scale 1/4,
    each query selecting one key by a margin of 40 nats): O is e4m3(code) / 4 bit for bit -- every such value is a bf16 value --, at most the
    other keys' leak of 2e-12 where that is +-0, and LSE the known score. Through the prefill and the decode (the plan splits the 4096 keys)."""
    T, G, page = 3, 4, 16
    k8, v8, ks, vs, want_v, score, cases = cs.all_codes_problem(D, T, G)
    want_v = want_v.to(BF)
    assert torch.equal(want_v.double(), v8.float().double().view(-1, D) * 0.25)
    assert pkg().fa2_decode_paged_multi_window_sink_bf16_fp8_plan(1, T, G, 1, 4096 // page, page, D, None)[0] >= 3
    for n, target, q in cases:
        pool = f8.make_pool(k8, v8, page, [n], seed=n)
        qb = q.to(BF)
        assert torch.equal(qb.float(), q.float())
        want = want_v[target.flatten()].view(1, T, G, D)
        zero = want == 0
        for name, (o, lse) in (("decode", run_multi(qb, pool, [n], ks, vs, None, None)),
                               ("prefill", run_prefill(qb[0], pool, [n], [0, T], ks, vs, None, None))):
            o, lse = o.view(1, T, G, D), lse.view(1, T, G)
            # bf16 has the exponent range of fp32: where fp16 flushes what the other keys leak to zero, bf16 keeps it. all_codes_problem bounds
            # that leak by 4096 e^-40 x 112 = 2e-12 (before v_scale = 1/4), which is what an expected +-0 may be
            wrong = int((bits(o)[~zero] != bits(want)[~zero]).sum()) + int((o[zero].float().abs() > 2e-12).sum())
            lerr = ((lse - score).abs() / score).max().item()
            print("%s D=%d len %d: %d of %d elements differ from e4m3(code) v_scale; LSE rel err %.2e" % (name, D, n, wrong, o.numel(), lerr))
            assert wrong == 0 and lerr <= 1e-5, (name, D, n, wrong, lerr)


# ---------------------------------------------------------------------------------------------------- against the bf16 entry

@pytest.mark.parametrize("D", DS)
def test_power_of_two_scales_against_the_bf16_sink_entry(built, dev, D):
    """With power-of-two scales the dequantised pools are bf16 tensors: the bf16 sink entry runs on them. Both entries meet the bound; whether the
    bits agree is printed (expected of the prefill: the same geometry and MFMA order; not of the decode, whose k-slot order differs)."""
    Hq, Hkv, page = 8, 2, 16
    qs, lens, bpool = sr.prefill_case(D, Hq, Hkv, page)
    ks, vs = fr.scales(Hkv, pow2=True)
    pool = fr.quantize_pools(bpool, ks, vs)
    dense = tuple(fr.dq(p, s).to(BF) for p, s in ((pool[0], ks), (pool[1], vs)))  # the pages of 0x7F are NaN in bf16 too
    assert all(torch.equal(torch.nan_to_num(d.double()), torch.nan_to_num(fr.dq(p, s))) for d, (p, s) in zip(dense, ((pool[0], ks), (pool[1], vs))))
    q, cu = sr.pack(qs)
    sinks = sr.prefill_sinks(Hq, 65)
    got = run_prefill(q, pool, lens, cu, ks, vs, 65, sinks)
    sib = sk.run_prefill(q, dense[0], dense[1], pool[2], lens, cu, 65, sinks)
    ref = fr.prefill(q, *pool, lens, cu, ks, vs, 65, sinks)
    note("prefill", check(*got, *ref, "pow2 prefill fp8 D=%d" % D))
    check(*sib, *ref, "pow2 prefill bf16 D=%d" % D)
    print("prefill D=%d: FP8 entry %s the bf16 sink entry bit for bit on the dequantised pools" % (D, "EQUALS" if same(got, sib) else "differs from"))
    q, lens, bpool = sr.decode_one_case(3, 4, D)
    ks, vs = fr.scales(sr.ONE_HKV, pow2=True)
    pool = fr.quantize_pools(bpool, ks, vs)
    dense = tuple(fr.dq(p, s).to(BF) for p, s in ((pool[0], ks), (pool[1], vs)))
    sinks = sr.sinks_mixed(q.shape[2], sr.ONE_W)
    got = run_multi(q, pool, lens, ks, vs, sr.ONE_W, sinks)
    sib = sk.run_multi(q, dense[0], dense[1], pool[2], lens, sr.ONE_W, sinks)
    ref = fr.decode(q, *pool, lens, ks, vs, sr.ONE_W, sinks)
    note("decode, one split", check(*got, *ref, "pow2 decode fp8 D=%d" % D))
    check(*sib, *ref, "pow2 decode bf16 D=%d" % D)
    print("decode D=%d: FP8 entry %s the bf16 sink entry bit for bit on the dequantised pools" % (D, "EQUALS" if same(got, sib) else "differs from"))


# ---------------------------------------------------------------------------------------------------- the gpt-oss layer shape

def test_gpt_oss_layer_pair_append_prefill_decode(built, dev):
    """Hq 64, Hkv 8, D 64, page 16: [130, 7] tokens appended with the half-split rotation into an empty FP8 pool (every byte 0x7F), a prefill at
    W = 128 (the sliding layers) and at None (the full layers), then one appended token and its T = 1 decode step. The reference quantises on the
    CPU (paged_bf16_fp8_reference.ref_append) and attends with the CPU-rotated q; the kernels' own pools and q_out feed the kernels."""
    c = pkg()
    Hq, Hkv, D, page, Nmax = 64, 8, 64, 16, 256
    g = torch.Generator().manual_seed(64)
    ks, vs = fr.scales(Hkv)
    sinks = sr.sinks_randn(Hq, 64) + 2.0
    Ts = [130, 7]
    B, mp = 2, Nmax // page
    P = B * mp + 1
    bt = torch.randperm(P - 1, generator=g).view(B, mp).to(torch.int32)
    table = c.kv_append_rope_table(Nmax, D)
    empty = torch.full((P, Hkv, page, D), fr.NAN_BYTE, dtype=torch.uint8).view(f8.F8)

    def append(kp8, vp8, k_new, v_new, q, lens, cu):
        """(the kernel's pools and q_out on the CPU, the CPU reference's pools and fp64 q rows)"""
        dk, dv = kp8.to(dev), vp8.to(dev)
        qo = torch.empty_like(q, device=dev)
        c.kv_append_paged_varlen_bf16_fp8(k_new.to(dev), v_new.to(dev), dk, dv, bt.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev),
                                          torch.tensor(cu, dtype=torch.int32, device=dev), ks.to(dev), vs.to(dev), q.to(dev), qo, table.to(dev),
                                          "half")
        torch.cuda.synchronize()
        kb, vb, _, rows, dead = fr.ref_append(k_new, v_new, kp8, vp8, bt, lens, cu, ks, vs, q, table, 1)
        assert not dead
        qr = torch.stack([r[5] for r in rows]).float().to(BF)  # the reference's q: the fp64 rotation rounded once
        return (dk.cpu(), dv.cpu(), qo.cpu()), (kb.view(f8.F8), vb.view(f8.F8), qr)

    k_new, v_new = (torch.randn(sum(Ts), Hkv, D, generator=g).to(BF) for _ in range(2))
    q = torch.randn(sum(Ts), Hq, D, generator=g).to(BF)
    cu = [0, Ts[0], sum(Ts)]
    (kp, vp, qo), (rk, rv, rq) = append(empty, empty, k_new, v_new, q, Ts, cu)
    assert torch.equal(f8.bits(vp), f8.bits(rv))  # V rows: byte for byte
    for W in (128, None):
        got = run_prefill(qo, (kp, vp, bt), Ts, cu, ks, vs, W, sinks)
        note("gpt-oss pair", check(*got, *fr.prefill(rq, rk, rv, bt, Ts, cu, ks, vs, W, sinks), "gpt-oss fp8 prefill W=%s" % W))
    step = [131, 8]
    k1, v1 = (torch.randn(2, Hkv, D, generator=g).to(BF) for _ in range(2))
    q1 = torch.randn(2, Hq, D, generator=g).to(BF)
    (kp, vp, qo), (rk, rv, rq) = append(kp, vp, k1, v1, q1, step, [0, 1, 2])
    for W in (128, None):
        got = run_multi(qo.view(2, 1, Hq, D), (kp, vp, bt), step, ks, vs, W, sinks)
        note("gpt-oss pair", check(*got, *fr.decode(rq.view(2, 1, Hq, D), rk, rv, bt, step, ks, vs, W, sinks), "gpt-oss fp8 decode W=%s" % W))


# ---------------------------------------------------------------------------------------------------- captured replay

def test_captured_append_and_decode_replay_the_eager_bits(built, dev):
    """append -> decode (T = 1) captured once in one graph on a single stream; replays with lengths, rows and table changed in place equal the
    eager pair bit for bit."""
    c = pkg()
    T, G, D = 1, 8, 64
    Hkv, Hq = sr.ONE_HKV, sr.ONE_HKV * G
    q, lens, pool, ks, vs = fr.decode_one_case(T, G, D)
    B = len(lens)
    kd, vd, bd, ksd, vsd = (t.to(dev) for t in (*pool, ks, vs))
    qd = q.view(B, Hq, D).to(dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev)
    snk = sr.sinks_randn(Hq, 1).to(dev)
    table = c.kv_append_rope_table(sr.ONE_NMAX, D, device=dev)
    kn, vn = (torch.randn(B, Hkv, D, generator=torch.Generator().manual_seed(5)).to(BF).to(dev) for _ in range(2))
    qr = torch.empty_like(qd)
    og, lg = torch.empty(B, 1, Hq, D, dtype=BF, device=dev), torch.empty(B, 1, Hq, dtype=torch.float32, device=dev)

    def step(o, lse):
        c.kv_append_paged_varlen_bf16_fp8(kn, vn, kd, vd, bd, sl, cu, ksd, vsd, qd, qr, table, "half")
        c.fa2_decode_paged_multi_window_sink_bf16_fp8(qr.view(B, 1, Hq, D), kd, vd, bd, sl, ksd, vsd, sr.ONE_W, snk, o, lse)

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
        qd.copy_(torch.randn(B, Hq, D, generator=gen).to(BF)), kn.copy_(torch.randn(B, Hkv, D, generator=gen).to(BF))
        vn.copy_(torch.randn(B, Hkv, D, generator=gen).to(BF))
        now = [max(n - 7 * (i + 1), 0) for n in lens]
        sl.copy_(torch.tensor(now, dtype=torch.int32))  # shorter: the table's live entries cover them
        p0, p1 = (now[0] - 1) // sr.PAGE, (now[1] - 1) // sr.PAGE  # the pages the new tokens of the first two sequences go to change places
        e0, e1 = int(bd[0, p0]), int(bd[1, p1])
        bd[0, p0], bd[1, p1] = e1, e0
        og.fill_(float("nan")), lg.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        oe, le = torch.full_like(og, float("nan")), torch.full_like(lg, float("nan"))
        step(oe, le)  # the append stores the same bytes again
        torch.cuda.synchronize()
        assert torch.equal(bits(og.cpu()), bits(oe.cpu())) and torch.equal(fbits(lg.cpu()), fbits(le.cpu())), i
        assert not bool(torch.isnan(og.float()).any())


def test_zz_report_the_largest_error_over_bound(built, dev):
    """Prints what DESIGN 4.4.11 and the reference module's docstring record; the siblings stayed below 0.4, and a ratio above 1 has failed its
    own test already."""
    for family, ratio in sorted(RATIOS.items()):
        print("largest O err / bound, %s: %.3f" % (family, ratio))
    assert all(r <= 1.0 for r in RATIOS.values())
