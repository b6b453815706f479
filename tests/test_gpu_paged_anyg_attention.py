"""GPU: the paged bf16 attention entries for any query-group size G = Hq / Hkv in 1 ... 16 -- cuda_learn_notes_amd.
fa2_prefill_paged_varlen_window_sink_anyg_bf16[_fp8] and fa2_decode_paged_multi_window_sink_anyg_bf16[_fp8] (csrc/*_anyg_*.cuh) --
against the families' own references: paged_sink_reference on bf16 pools, paged_bf16_fp8_reference on the dequantised e4m3 pools. No new
tolerance: O within paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol per head, -inf LSE entries and zero rows
exactly (test_gpu_paged_sink_attention.check). The cases are tests/paged_anyg_cases.py's, which tests/test_paged_anyg_surface.py shows to be
sensitive to the three wrong row maps. Beyond parity, bit for bit: for G in {1, 2, 4, 8} the power-of-two siblings' O and LSE, a packed sequence
is its B = 1 call, sinks of -inf are sinks = None. Every parity case prints err / bound before it asserts (pytest -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import paged_anyg_cases as ac  # noqa: E402
import paged_bf16_fp8_reference as fr  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import test_gpu_paged_bf16_fp8_attention as f8t  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DS = [64, 128]
FAMILIES = ["bf16", "fp8"]
O_FILL, L_FILL = sk.O_FILL, sk.L_FILL
NEG_INF = float("-inf")
bits, fbits, check, same = sk.bits, sk.fbits, sk.check, f8t.same
RATIOS = {}  # the largest err / bound per group of cases, printed by the last test of the file


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


class Family:
    """One of the two pool formats: how a bf16 pool becomes this family's, how the new entries and the siblings are called, and the reference."""

    def __init__(self, name):
        self.fp8 = name == "fp8"

    def pool(self, pool, Hkv):
        if not self.fp8:
            return pool, ()
        p8, ks, vs = ac.to_fp8(pool, Hkv)
        return p8, (ks, vs)

    def prefill(self, q, pool, sc, lens, cu, W, sinks, sibling=False, dev="cuda"):
        c = pkg()
        fn = getattr(c, "fa2_prefill_paged_varlen_window_sink_%sbf16%s" % ("" if sibling else "anyg_", "_fp8" if self.fp8 else ""))
        qd, kd, vd, bd = (t.to(dev) for t in (q, *pool))
        sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
        cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
        o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
        lse = torch.full(qd.shape[:2], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
        fn(qd, kd, vd, bd, sl, cd, *(s.to(dev) for s in sc), W, None if sinks is None else sinks.to(dev), o, lse)
        torch.cuda.synchronize()
        return o.cpu(), lse.cpu()

    def decode(self, q, pool, sc, lens, W, sinks, sibling=False, dev="cuda"):
        c = pkg()
        name = "fa2_decode_paged_multi_window_sink_%sbf16%s" % ("" if sibling else "anyg_", "_fp8" if self.fp8 else "")
        qd, kd, vd, bd = (t.to(dev) for t in (q, *pool))
        sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
        o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
        lse = torch.full(qd.shape[:3], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
        B, T, Hq, D = q.shape
        need = getattr(c, name + "_plan")(B, T, Hq, pool[0].shape[1], pool[2].shape[1], pool[0].shape[2], D, W)[2]  # sized from the entry's own plan
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        getattr(c, name)(qd, kd, vd, bd, sl, *(s.to(dev) for s in sc), W, None if sinks is None else sinks.to(dev), o, lse, ws)
        torch.cuda.synchronize()
        return o.cpu(), lse.cpu()

    def ref_prefill(self, q, pool, sc, lens, cu, W, sinks):
        if self.fp8:
            return fr.prefill(q, *pool, lens, cu, *sc, W, sinks)
        return sr.prefill(q, *pool, lens, cu, W, sr.sinks_const(q.shape[1], NEG_INF) if sinks is None else sinks)

    def ref_decode(self, q, pool, sc, lens, W, sinks):
        if self.fp8:
            return fr.decode(q, *pool, lens, *sc, W, sinks)
        return sr.decode(q, *pool, lens, W, sr.sinks_const(q.shape[2], NEG_INF) if sinks is None else sinks)


# ---------------------------------------------------------------------------------------------------- 1. prefill, rows that straddle tiles

@pytest.mark.parametrize("page", ac.P1_PAGES)
@pytest.mark.parametrize("G", ac.GROUPS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_prefill_rows_that_straddle_tiles(built, dev, fam, D, G, page):
    f = Family(fam)
    q, cu, lens, bpool = ac.prefill_case(D, G, page)
    Hq = ac.P1_HKV * G
    pool, sc = f.pool(bpool, ac.P1_HKV)
    for W in ac.P1_WINDOWS:
        none = None
        for name, sinks in (("none", None), ("mixed", ac.sinks_for(Hq, 33))):
            got = f.prefill(q, pool, sc, lens, cu, W, sinks)
            note("prefill, one sequence", check(*got, *f.ref_prefill(q, pool, sc, lens, cu, W, sinks),
                                                "%s prefill D=%d G=%d page=%d W=%s %s" % (fam, D, G, page, W, name)))
            none = none or got
        assert same(f.prefill(q, pool, sc, lens, cu, W, sr.sinks_const(Hq, NEG_INF)), none), (fam, D, G, page, W)  # 7: -inf is None


# ---------------------------------------------------------------------------------------------------- 2. packed ragged prefill

@pytest.mark.parametrize("G", ac.P2_G)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_packed_ragged_prefill_and_every_sequence_alone(built, dev, fam, D, G):
    f = Family(fam)
    qs, lens, bpool = ac.ragged_case(D, G)
    Hq, W = ac.P2_HKV * G, ac.P2_W
    pool, sc = f.pool(bpool, ac.P2_HKV)
    q, cu = sr.pack(qs, 3, 5)
    seq = slice(cu[0], cu[-1])
    sinks = ac.sinks_for(Hq, W)
    o, lse = f.prefill(q, pool, sc, lens, cu, W, sinks)
    for sl in (slice(0, cu[0]), slice(cu[-1], None)):  # the rows of no sequence are untouched
        assert bool((bits(o[sl]) == O_FILL).all()) and bool((fbits(lse[sl]) == L_FILL).all())
    ro, rl, emul = f.ref_prefill(q, pool, sc, lens, cu, W, sinks)
    note("prefill, packed", check(o[seq], lse[seq], ro[seq], rl[seq], emul[seq], "%s ragged prefill D=%d G=%d" % (fam, D, G)))
    kp, vp, bt = pool
    for b, qb in enumerate(qs):  # every sequence alone, B = 1: the packed run's bits
        t = qb.shape[0]
        q1 = torch.cat((qb, torch.full((1,) + tuple(qb.shape[1:]), 2.0 ** 100, dtype=BF)))
        o1, l1 = f.prefill(q1, (kp, vp, bt[b:b + 1].contiguous()), sc, [lens[b]], [0, t], W, sinks)
        assert torch.equal(bits(o1[:t]), bits(o[cu[b]:cu[b + 1]])) and torch.equal(fbits(l1[:t]), fbits(lse[cu[b]:cu[b + 1]])), (fam, D, G, b)
        assert bool((bits(o1[t:]) == O_FILL).all())


# ---------------------------------------------------------------------------------------------------- 3. decode, one split

@pytest.mark.parametrize("TG", ac.D3_TG, ids=lambda tg: "T%dxG%d" % tg)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_decode_one_split(built, dev, fam, D, TG):
    f = Family(fam)
    T, G = TG
    q, lens, bpool = ac.decode_one_case(T, G, D)
    Hq = ac.D3_HKV * G
    pool, sc = f.pool(bpool, ac.D3_HKV)
    for W in ac.D3_WINDOWS:
        assert pkg().fa2_decode_paged_multi_window_sink_anyg_bf16_plan(len(lens), T, Hq, ac.D3_HKV, ac.D3_NMAX // ac.PAGE, ac.PAGE, D, W)[0] == 1
        none = None
        for name, sinks in (("none", None), ("mixed", ac.sinks_for(Hq, 33))):
            got = f.decode(q, pool, sc, lens, W, sinks)
            note("decode, one split", check(*got, *f.ref_decode(q, pool, sc, lens, W, sinks),
                                            "%s decode S=1 D=%d T=%d G=%d W=%s %s" % (fam, D, T, G, W, name)))
            none = none or got
        assert bool((none[0][0] == 0).all()) and bool((none[1][0] == NEG_INF).all())  # 7: len 0 sees no key
        assert same(f.decode(q, pool, sc, lens, W, sr.sinks_const(Hq, NEG_INF)), none), (fam, D, T, G, W)


# ---------------------------------------------------------------------------------------------------- 4. decode, several splits

@pytest.mark.parametrize("TG", ac.D4_TG, ids=lambda tg: "T%dxG%d" % tg)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_decode_several_splits(built, dev, fam, D, TG):
    f = Family(fam)
    T, G = TG
    for W in ac.D4_WINDOWS:
        assert pkg().fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan(1, T, G, 1, ac.D4_NMAX // ac.PAGE, ac.PAGE, D, W)[0] > 1
        for n in ac.D4_LENS:
            q, lens, bpool = ac.decode_split_case(T, G, D, n)
            pool, sc = f.pool(bpool, 1)
            none = None
            for name, sinks in (("none", None), ("mixed", ac.sinks_for(G, n if W is None else min(W, n)))):
                got = f.decode(q, pool, sc, lens, W, sinks)
                note("decode, several splits", check(*got, *f.ref_decode(q, pool, sc, lens, W, sinks),
                                                     "%s decode S>1 D=%d T=%d G=%d W=%s len=%d %s" % (fam, D, T, G, W, n, name)))
                none = none or got
            assert same(f.decode(q, pool, sc, lens, W, sr.sinks_const(G, NEG_INF)), none), (fam, D, T, G, W, n)


# ---------------------------------------------------------------------------------------------------- 5. the siblings' bits

@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_powers_of_two_give_the_siblings_bits(built, dev, fam, D):
    """The evidence that the division changed nothing else: O and LSE bit for bit. The bf16 sibling has no sinks = None, so it runs with sinks; the
    FP8 sibling runs with and without."""
    f = Family(fam)
    sets = lambda Hq, n: ((ac.sinks_for(Hq, n),) + ((None,) if f.fp8 else ()))  # noqa: E731
    for G in ac.S5_PREFILL_G:
        q, cu, lens, bpool = ac.prefill_case(D, G, 16)
        pool, sc = f.pool(bpool, ac.P1_HKV)
        for W in ac.P1_WINDOWS:
            for sinks in sets(ac.P1_HKV * G, 33):
                assert same(f.prefill(q, pool, sc, lens, cu, W, sinks), f.prefill(q, pool, sc, lens, cu, W, sinks, sibling=True)), (fam, D, G, W)
    for T, G in ac.S5_DECODE_TG:
        q, lens, bpool = ac.decode_one_case(T, G, D)
        pool, sc = f.pool(bpool, ac.D3_HKV)
        for W in ac.D3_WINDOWS:
            for sinks in sets(ac.D3_HKV * G, 33):
                assert same(f.decode(q, pool, sc, lens, W, sinks), f.decode(q, pool, sc, lens, W, sinks, sibling=True)), (fam, D, T, G, W)
        q, lens, bpool = ac.decode_split_case(T, G, D, 4096)
        pool, sc = f.pool(bpool, 1)
        for W in ac.D4_WINDOWS:
            assert pkg().fa2_decode_paged_multi_window_sink_anyg_bf16_plan(1, T, G, 1, ac.D4_NMAX // ac.PAGE, ac.PAGE, D, W)[0] > 1
            for sinks in sets(G, 1000):
                assert same(f.decode(q, pool, sc, lens, W, sinks), f.decode(q, pool, sc, lens, W, sinks, sibling=True)), (fam, D, T, G, W, "split")
    for G in (1, 2):  # the two smallest, on the packed ragged shape
        Hkv = ac.P2_HKV
        g = torch.Generator().manual_seed(G + D)
        qs = tuple(torch.randn(t, Hkv * G, D, generator=g).to(BF) for t in ac.P2_T)
        _, lens, bpool = ac.ragged_case(D, 3)
        pool, sc = f.pool(bpool, Hkv)
        q, cu = sr.pack(qs)
        sinks = ac.sinks_for(Hkv * G, 33)
        assert same(f.prefill(q, pool, sc, lens, cu, 33, sinks), f.prefill(q, pool, sc, lens, cu, 33, sinks, sibling=True)), (fam, D, G)


# ---------------------------------------------------------------------------------------------------- 6. a serving chain at 14 / 2 heads

@pytest.mark.parametrize("fam", FAMILIES)
def test_serving_chain_at_seven_query_heads_per_kv_head(built, dev, fam):
    """Qwen2.5-7B's ratio scaled down: Hq 14, Hkv 2, D 128, page 16. The EXISTING packed append (rope 'none': rows copied, or quantised) fills an
    empty pool with [37, 5] tokens, the new prefill attends; then one appended token and the T = 1 decode, then three and the T = 3 decode. The
    append is checked against the rows it was given (bf16: bit for bit; FP8: paged_bf16_fp8_reference.ref_append byte for byte)."""
    c, f = pkg(), Family(fam)
    Hq, Hkv, D, page, Nmax = 14, 2, 128, 16, 64
    g = torch.Generator().manual_seed(14)
    B, mp = 2, Nmax // page
    P = B * mp + 1
    bt = torch.randperm(P - 1, generator=g).view(B, mp).to(torch.int32)
    sc = fr.scales(Hkv) if f.fp8 else ()
    sinks = ac.sinks_for(Hq, 33)
    if f.fp8:
        kp = torch.full((P, Hkv, page, D), fr.NAN_BYTE, dtype=torch.uint8).view(f8.F8)
    else:
        kp = torch.full((P, Hkv, page, D), float("nan"), dtype=BF)
    kp, vp = kp.to(dev), kp.clone().to(dev)
    rk, rv = kp.cpu(), vp.cpu()  # the reference's pools
    lens = [0, 0]
    for step, Ts in enumerate(([37, 5], [1, 1], [3, 3])):
        cu = [0, Ts[0], Ts[0] + Ts[1]]
        lens = [n + t for n, t in zip(lens, Ts)]
        k_new, v_new = (torch.randn(cu[-1], Hkv, D, generator=g).to(BF) for _ in range(2))
        q = torch.randn(cu[-1], Hq, D, generator=g).to(BF)
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        cd = torch.tensor(cu, dtype=torch.int32, device=dev)
        append = c.kv_append_paged_varlen_bf16_fp8 if f.fp8 else c.kv_append_paged_varlen_bf16
        append(k_new.to(dev), v_new.to(dev), kp, vp, bt.to(dev), sl, cd, *(s.to(dev) for s in sc))
        torch.cuda.synchronize()
        if f.fp8:
            kb, vb, _, _, dead = fr.ref_append(k_new, v_new, rk, rv, bt, lens, cu, *sc, None, None, 0)
            assert not dead
            rk, rv = kb.view(f8.F8), vb.view(f8.F8)
            assert torch.equal(f8.bits(kp.cpu()), f8.bits(rk)) and torch.equal(f8.bits(vp.cpu()), f8.bits(rv)), step
        else:
            rk, rv = rk.clone(), rv.clone()
            for b in range(B):
                for t in range(Ts[b]):
                    pos = lens[b] - Ts[b] + t
                    rk[bt[b, pos // page], :, pos % page], rv[bt[b, pos // page], :, pos % page] = k_new[cu[b] + t], v_new[cu[b] + t]
            assert torch.equal(bits(kp.cpu()), bits(rk)) and torch.equal(bits(vp.cpu()), bits(rv)), step
        pool = (kp.cpu(), vp.cpu(), bt)
        for W in (None, 33):
            if step == 0:
                got = f.prefill(q, pool, sc, lens, cu, W, sinks)
                note("serving chain", check(*got, *f.ref_prefill(q, (rk, rv, bt), sc, lens, cu, W, sinks), "%s chain prefill W=%s" % (fam, W)))
            else:
                q4 = q.view(B, Ts[0], Hq, D)
                got = f.decode(q4, pool, sc, lens, W, sinks)
                note("serving chain", check(*got, *f.ref_decode(q4, (rk, rv, bt), sc, lens, W, sinks), "%s chain decode T=%d W=%s" % (fam, Ts[0], W)))


# ---------------------------------------------------------------------------------------------------- 7. rows that see no key

@pytest.mark.parametrize("fam", FAMILIES)
def test_rows_that_see_no_key_stay_zero_with_lse_minus_inf(built, dev, fam):
    """The 45-token sequence with a length of 20: its first 25 tokens, 25 G rows that cross tiles of 16 and of 128, see no key -- O = 0 and
    LSE = -inf whatever the sink -- and the tile that holds only such rows takes the early return."""
    f = Family(fam)
    for D, G in ((64, 7), (128, 12)):
        q, cu, _, bpool = ac.prefill_case(D, G, 16)
        lens = [20]
        pool, sc = f.pool((bpool[0], bpool[1], bpool[2]), ac.P1_HKV)
        for sinks in (None, ac.sinks_for(ac.P1_HKV * G, 20)):
            o, lse = f.prefill(q, pool, sc, lens, cu, 33, sinks)
            assert bool((bits(o[:25]) == 0).all()) and bool((lse[:25] == NEG_INF).all()) and bool(torch.isfinite(lse[25:]).all())
            note("prefill, one sequence", check(o, lse, *f.ref_prefill(q, pool, sc, lens, cu, 33, sinks), "%s dead rows D=%d G=%d" % (fam, D, G)))


def test_zz_report_the_largest_error_over_bound(built, dev):
    """Prints what DESIGN 4.4.13 records; the siblings stayed below 0.4, and a ratio above 1 has failed its own test already."""
    for group, ratio in sorted(RATIOS.items()):
        print("largest O err / bound, %s: %.3f" % (group, ratio))
    assert all(r <= 1.0 for r in RATIOS.values())
