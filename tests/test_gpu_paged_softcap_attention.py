"""GPU: the paged bf16 attention entries with a softmax scale and logit soft-capping -- cuda_learn_notes_amd.
fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16[_fp8] and fa2_decode_paged_multi_window_sink_softcap_anyg_bf16[_fp8]
(csrc/*_softcap_anyg_*.cuh) -- against tests/paged_softcap_reference.py: the fp64 reference and the bf16 emulation of the
families with `scale` and `cap`. No new tolerance: O within paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol
per head, -inf LSE entries and zero rows exactly (test_gpu_paged_sink_attention.check). The cases are tests/paged_anyg_cases.py's shapes with q x 4
and a cap of 2, which tests/test_paged_softcap_surface.py shows to be sensitive to the six defects of the reference module; the cap and the scale
are each on and off. Beyond parity, bit for bit: scale = cap = None gives the any-G entries' O and LSE, a packed sequence is its B = 1 call,
sinks of -inf are sinks = None, rows that see no key are O = 0 and LSE = -inf, and at D = 64 a scale of 0.125 is None. Every parity case prints
err / bound before it asserts (pytest -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import paged_anyg_cases as ac  # noqa: E402
import paged_bf16_fp8_reference as fr  # noqa: E402
import paged_softcap_reference as cr  # noqa: E402
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
    """One of the two pool formats: how a bf16 pool becomes this family's, how the new entries and the any-G entries are called, the reference."""

    def __init__(self, name):
        self.fp8 = name == "fp8"

    def pool(self, pool, Hkv):
        if not self.fp8:
            return pool, ()
        p8, ks, vs = ac.to_fp8(pool, Hkv)
        return p8, (ks, vs)

    def prefill(self, q, pool, sc, lens, cu, W, sinks, scale=None, cap=None, anyg=False, dev="cuda"):
        c = pkg()
        fn = getattr(c, "fa2_prefill_paged_varlen_window_sink_%sanyg_bf16%s" % ("" if anyg else "softcap_", "_fp8" if self.fp8 else ""))
        qd, kd, vd, bd = (t.to(dev) for t in (q, *pool))
        sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
        cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
        o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
        lse = torch.full(qd.shape[:2], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
        fn(qd, kd, vd, bd, sl, cd, *(s.to(dev) for s in sc), W, None if sinks is None else sinks.to(dev), *(() if anyg else (scale, cap)), o, lse)
        torch.cuda.synchronize()
        return o.cpu(), lse.cpu()

    def decode(self, q, pool, sc, lens, W, sinks, scale=None, cap=None, anyg=False, dev="cuda"):
        c = pkg()
        name = "fa2_decode_paged_multi_window_sink_%sanyg_bf16%s" % ("" if anyg else "softcap_", "_fp8" if self.fp8 else "")
        qd, kd, vd, bd = (t.to(dev) for t in (q, *pool))
        sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
        o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
        lse = torch.full(qd.shape[:3], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
        B, T, Hq, D = q.shape
        need = getattr(c, name + "_plan")(B, T, Hq, pool[0].shape[1], pool[2].shape[1], pool[0].shape[2], D, W)[2]  # sized from the entry's own plan
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        getattr(c, name)(qd, kd, vd, bd, sl, *(s.to(dev) for s in sc), W, None if sinks is None else sinks.to(dev),
                         *(() if anyg else (scale, cap)), o, lse, ws)
        torch.cuda.synchronize()
        return o.cpu(), lse.cpu()

    def _kw(self, sc):
        return {"ks": sc[0], "vs": sc[1]} if self.fp8 else {}

    def ref_prefill(self, q, pool, sc, lens, cu, W, sinks, scale, cap):
        return cr.prefill(q, *pool, lens, cu, W, sinks, scale, cap, **self._kw(sc))

    def ref_decode(self, q, pool, sc, lens, W, sinks, scale, cap):
        return cr.decode(q, *pool, lens, W, sinks, scale, cap, **self._kw(sc))


# ---------------------------------------------------------------------------------------------------- 1. prefill, rows that straddle tiles

@pytest.mark.parametrize("page", cr.P1_PAGES)
@pytest.mark.parametrize("G", cr.P1_G)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_prefill_rows_that_straddle_tiles(built, dev, fam, D, G, page):
    f = Family(fam)
    q, cu, lens, bpool = cr.prefill_case(D, G, page)
    Hq = ac.P1_HKV * G
    pool, sc = f.pool(bpool, ac.P1_HKV)
    sinks = ac.sinks_for(Hq, 33)
    for W in cr.P1_WINDOWS:
        for name, scale, cap in cr.configs(D):
            got = f.prefill(q, pool, sc, lens, cu, W, sinks, scale, cap)
            note("prefill, one sequence, " + name, check(*got, *f.ref_prefill(q, pool, sc, lens, cu, W, sinks, scale, cap),
                                                         "%s prefill D=%d G=%d page=%d W=%s %s" % (fam, D, G, page, W, name)))
        none = f.prefill(q, pool, sc, lens, cu, W, None, cr.scale_for(D), cr.CAP)  # sinks of -inf are sinks = None, with the cap on
        note("prefill, one sequence, scale+cap", check(*none, *f.ref_prefill(q, pool, sc, lens, cu, W, None, cr.scale_for(D), cr.CAP),
                                                       "%s prefill D=%d G=%d page=%d W=%s no sinks" % (fam, D, G, page, W)))
        assert same(f.prefill(q, pool, sc, lens, cu, W, sr.sinks_const(Hq, NEG_INF), cr.scale_for(D), cr.CAP), none), (fam, D, G, page, W)


# ---------------------------------------------------------------------------------------------------- 2. packed ragged prefill

@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_packed_ragged_prefill_and_every_sequence_alone(built, dev, fam, D):
    f = Family(fam)
    G = cr.P2_G
    qs, lens, bpool = cr.ragged_case(D, G)
    Hq, W = ac.P2_HKV * G, ac.P2_W
    pool, sc = f.pool(bpool, ac.P2_HKV)
    q, cu = sr.pack(qs, 3, 5)
    seq = slice(cu[0], cu[-1])
    sinks = ac.sinks_for(Hq, W)
    for name, scale, cap in cr.configs(D):
        o, lse = f.prefill(q, pool, sc, lens, cu, W, sinks, scale, cap)
        for sl in (slice(0, cu[0]), slice(cu[-1], None)):  # the rows of no sequence are untouched
            assert bool((bits(o[sl]) == O_FILL).all()) and bool((fbits(lse[sl]) == L_FILL).all())
        ro, rl, emul = f.ref_prefill(q, pool, sc, lens, cu, W, sinks, scale, cap)
        note("prefill, packed, " + name, check(o[seq], lse[seq], ro[seq], rl[seq], emul[seq], "%s ragged prefill D=%d G=%d %s" % (fam, D, G, name)))
    kp, vp, bt = pool
    for b, qb in enumerate(qs):  # every sequence alone, B = 1: the packed run's bits, with the cap on (o, lse: the last config's)
        t = qb.shape[0]
        q1 = torch.cat((qb, torch.full((1,) + tuple(qb.shape[1:]), 2.0 ** 100, dtype=BF)))
        o1, l1 = f.prefill(q1, (kp, vp, bt[b:b + 1].contiguous()), sc, [lens[b]], [0, t], W, sinks, scale, cap)
        assert torch.equal(bits(o1[:t]), bits(o[cu[b]:cu[b + 1]])) and torch.equal(fbits(l1[:t]), fbits(lse[cu[b]:cu[b + 1]])), (fam, D, G, b)
        assert bool((bits(o1[t:]) == O_FILL).all())


# ---------------------------------------------------------------------------------------------------- 3. decode, one split

@pytest.mark.parametrize("TG", cr.D3_TG, ids=lambda tg: "T%dxG%d" % tg)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_decode_one_split(built, dev, fam, D, TG):
    f = Family(fam)
    T, G = TG
    q, lens, bpool = cr.decode_one_case(T, G, D)
    Hq = ac.D3_HKV * G
    pool, sc = f.pool(bpool, ac.D3_HKV)
    sinks = ac.sinks_for(Hq, 33)
    for W in ac.D3_WINDOWS:
        assert pkg().fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(len(lens), T, Hq, ac.D3_HKV, ac.D3_NMAX // ac.PAGE, ac.PAGE, D, W)[0] == 1
        for name, scale, cap in cr.configs(D):
            got = f.decode(q, pool, sc, lens, W, sinks, scale, cap)
            note("decode, one split, " + name, check(*got, *f.ref_decode(q, pool, sc, lens, W, sinks, scale, cap),
                                                     "%s decode S=1 D=%d T=%d G=%d W=%s %s" % (fam, D, T, G, W, name)))
        none = f.decode(q, pool, sc, lens, W, None, cr.scale_for(D), cr.CAP)
        assert bool((none[0][0] == 0).all()) and bool((none[1][0] == NEG_INF).all())  # len 0 sees no key, with the cap on
        assert same(f.decode(q, pool, sc, lens, W, sr.sinks_const(Hq, NEG_INF), cr.scale_for(D), cr.CAP), none), (fam, D, T, G, W)


# ---------------------------------------------------------------------------------------------------- 4. decode, several splits

@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_decode_several_splits(built, dev, fam, D):
    f = Family(fam)
    T, G = cr.D4_TG
    for W in cr.D4_WINDOWS:
        assert pkg().fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan(1, T, G, 1, ac.D4_NMAX // ac.PAGE, ac.PAGE, D, W)[0] > 1
        for n in cr.D4_LENS:
            q, lens, bpool = cr.decode_split_case(T, G, D, n)
            pool, sc = f.pool(bpool, 1)
            sinks = ac.sinks_for(G, n if W is None else min(W, n))
            for name, scale, cap in cr.configs(D):
                got = f.decode(q, pool, sc, lens, W, sinks, scale, cap)
                note("decode, several splits, " + name, check(*got, *f.ref_decode(q, pool, sc, lens, W, sinks, scale, cap),
                                                              "%s decode S>1 D=%d T=%d G=%d W=%s len=%d %s" % (fam, D, T, G, W, n, name)))
            none = f.decode(q, pool, sc, lens, W, None, None, cr.CAP)
            assert same(f.decode(q, pool, sc, lens, W, sr.sinks_const(G, NEG_INF), None, cr.CAP), none), (fam, D, T, G, W, n)


# ---------------------------------------------------------------------------------------------------- 5. the any-G entries' bits

@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_no_scale_and_no_cap_give_the_any_g_entries_bits(built, dev, fam, D):
    """The evidence that CAP = false with the default multiplier is the any-G path: O and LSE bit for bit, on the prefill, on the decode with one
    split and on the decode with several, with and without sinks."""
    f = Family(fam)
    for G in cr.S5_G:
        q, cu, lens, bpool = cr.prefill_case(D, G, 16)
        pool, sc = f.pool(bpool, ac.P1_HKV)
        for W in cr.P1_WINDOWS:
            for sinks in (ac.sinks_for(ac.P1_HKV * G, 33), None):
                assert same(f.prefill(q, pool, sc, lens, cu, W, sinks), f.prefill(q, pool, sc, lens, cu, W, sinks, anyg=True)), (fam, D, G, W)
        T = 3 if G == 3 else 8
        q, lens, bpool = cr.decode_one_case(*((1, 3) if G == 3 else (8, 8)), D)
        pool, sc = f.pool(bpool, ac.D3_HKV)
        for W in ac.D3_WINDOWS:
            for sinks in (ac.sinks_for(ac.D3_HKV * G, 33), None):
                assert same(f.decode(q, pool, sc, lens, W, sinks), f.decode(q, pool, sc, lens, W, sinks, anyg=True)), (fam, D, G, W)
        q, lens, bpool = ac.decode_split_case(T, G, D, 4096)
        pool, sc = f.pool(bpool, 1)
        for W in cr.D4_WINDOWS:
            assert pkg().fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(1, T, G, 1, ac.D4_NMAX // ac.PAGE, ac.PAGE, D, W)[0] > 1
            for sinks in (ac.sinks_for(G, 1000), None):
                assert same(f.decode(q, pool, sc, lens, W, sinks), f.decode(q, pool, sc, lens, W, sinks, anyg=True)), (fam, D, G, W, "split")


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_scale_of_one_eighth_is_none_at_head_dim_64(built, dev, fam):
    """1 / sqrt(64) is a float: (float)(0.125 log2 e) and (float)(log2 e / sqrt(64)) are one number, and so are the results, cap or not. D = 128
    has no exactly representable 1 / sqrt(D): no such claim there."""
    f = Family(fam)
    q, cu, lens, bpool = cr.prefill_case(64, 3, 16)
    pool, sc = f.pool(bpool, ac.P1_HKV)
    sinks = ac.sinks_for(ac.P1_HKV * 3, 33)
    for cap in (None, cr.CAP):
        assert same(f.prefill(q, pool, sc, lens, cu, 33, sinks, 0.125, cap), f.prefill(q, pool, sc, lens, cu, 33, sinks, None, cap)), (fam, cap)
    q, lens, bpool = cr.decode_one_case(8, 8, 64)
    pool, sc = f.pool(bpool, ac.D3_HKV)
    sinks = ac.sinks_for(ac.D3_HKV * 8, 33)
    for cap in (None, cr.CAP):
        assert same(f.decode(q, pool, sc, lens, 33, sinks, 0.125, cap), f.decode(q, pool, sc, lens, 33, sinks, None, cap)), (fam, cap)


# ---------------------------------------------------------------------------------------------------- 6. the three models' numbers, bad arguments

@pytest.mark.parametrize("model", sorted(cr.MODELS))
@pytest.mark.parametrize("fam", FAMILIES)
def test_the_models_numbers_on_randn_data(built, dev, fam, model):
    """Plain parity at D = 128 on randn data (the cap of 30 or 50 hardly acts on it): Gemma-2-27B's scale 144^-1/2 with cap 50, Gemma-3-27B's
    168^-1/2 without a cap under a window, Grok-1's G = 6 with cap 30 -- the prefill of 45 tokens and a decode of T = 3."""
    f = Family(fam)
    G, scale, cap, W = cr.MODELS[model]
    D = 128
    q, cu, lens, bpool = ac.prefill_case(D, G, 16)
    pool, sc = f.pool(bpool, ac.P1_HKV)
    sinks = None if model != "gemma-3-27b" else ac.sinks_for(ac.P1_HKV * G, 33)
    got = f.prefill(q, pool, sc, lens, cu, W, sinks, scale, cap)
    note("models", check(*got, *f.ref_prefill(q, pool, sc, lens, cu, W, sinks, scale, cap), "%s %s prefill" % (fam, model)))
    q4 = q[:15].reshape(5, 3, *q.shape[1:]).contiguous()
    _, dlens, dpool = ac.decode_one_case(3, 5, D)
    pool, sc = f.pool(dpool, ac.D3_HKV)
    got = f.decode(q4, pool, sc, dlens, W, sinks, scale, cap)
    note("models", check(*got, *f.ref_decode(q4, pool, sc, dlens, W, sinks, scale, cap), "%s %s decode T=3" % (fam, model)))


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_huge_cap_is_no_cap_and_a_tiny_cap_gives_no_nan(built, dev, fam):
    f = Family(fam)
    D, G = 128, 3
    q, cu, lens, bpool = cr.prefill_case(D, G, 16)
    pool, sc = f.pool(bpool, ac.P1_HKV)
    sinks = ac.sinks_for(ac.P1_HKV * G, 33)
    ref = f.ref_prefill(q, pool, sc, lens, cu, 33, sinks, None, None)
    note("cap 1e30", check(*f.prefill(q, pool, sc, lens, cu, 33, sinks, None, 1e30), *ref, "%s prefill cap 1e30 against no cap" % fam))
    o, lse = f.prefill(q, pool, sc, lens, cu, 33, sinks, None, 1e-30)
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any())
    note("cap 1e-30", check(o, lse, *f.ref_prefill(q, pool, sc, lens, cu, 33, sinks, None, 1e-30), "%s prefill cap 1e-30" % fam))
    q, lens, bpool = cr.decode_one_case(4, 16, D)
    pool, sc = f.pool(bpool, ac.D3_HKV)
    sinks = ac.sinks_for(ac.D3_HKV * 16, 33)
    ref = f.ref_decode(q, pool, sc, lens, None, sinks, None, None)
    note("cap 1e30", check(*f.decode(q, pool, sc, lens, None, sinks, None, 1e30), *ref, "%s decode cap 1e30 against no cap" % fam))
    o, lse = f.decode(q, pool, sc, lens, None, sinks, None, 1e-30)
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any())


# ---------------------------------------------------------------------------------------------------- 7. rows that see no key

@pytest.mark.parametrize("fam", FAMILIES)
def test_rows_that_see_no_key_stay_zero_with_lse_minus_inf(built, dev, fam):
    """The any-G file's len-20 case with the cap on: the first 25 of the 45 tokens see no key -- O = 0 and LSE = -inf whatever the sink."""
    f = Family(fam)
    for D, G in ((64, 7), (128, 12)):
        q, cu, _, bpool = cr.prefill_case(D, G, 16)
        lens = [20]
        pool, sc = f.pool(bpool, ac.P1_HKV)
        for sinks in (None, ac.sinks_for(ac.P1_HKV * G, 20)):
            o, lse = f.prefill(q, pool, sc, lens, cu, 33, sinks, cr.scale_for(D), cr.CAP)
            assert bool((bits(o[:25]) == 0).all()) and bool((lse[:25] == NEG_INF).all()) and bool(torch.isfinite(lse[25:]).all())
            note("prefill, one sequence, scale+cap", check(o, lse, *f.ref_prefill(q, pool, sc, lens, cu, 33, sinks, cr.scale_for(D), cr.CAP),
                                                           "%s dead rows D=%d G=%d" % (fam, D, G)))


# ---------------------------------------------------------------------------------------------------- 8. a serving chain at Gemma-2's numbers

@pytest.mark.parametrize("fam", FAMILIES)
def test_serving_chain_with_gemma_2_scale_and_cap(built, dev, fam):
    """4 / 2 heads, D 128, page 16, scale 144^-1/2, cap 50. The EXISTING packed append (rope 'none') fills an empty pool with [37, 5] tokens, the
    new prefill attends; then one appended token and the T = 1 decode, then three and the T = 3 decode; W in {None, 33}. q x 4 makes the cap act."""
    c, f = pkg(), Family(fam)
    Hq, Hkv, D, page, Nmax = 4, 2, 128, 16, 64
    scale, cap = 144 ** -0.5, 50.0
    g = torch.Generator().manual_seed(27)
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
    lens = [0, 0]
    for step, Ts in enumerate(([37, 5], [1, 1], [3, 3])):
        cu = [0, Ts[0], Ts[0] + Ts[1]]
        lens = [n + t for n, t in zip(lens, Ts)]
        k_new, v_new = ((torch.randn(cu[-1], Hkv, D, generator=g) * 4).to(BF) for _ in range(2))
        q = (torch.randn(cu[-1], Hq, D, generator=g) * 4).to(BF)
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        cd = torch.tensor(cu, dtype=torch.int32, device=dev)
        append = c.kv_append_paged_varlen_bf16_fp8 if f.fp8 else c.kv_append_paged_varlen_bf16
        append(k_new.to(dev), v_new.to(dev), kp, vp, bt.to(dev), sl, cd, *(s.to(dev) for s in sc))
        torch.cuda.synchronize()
        pool = (kp.cpu(), vp.cpu(), bt)  # the append entries have their own tests; the reference reads the pools they wrote
        for W in (None, 33):
            if step == 0:
                got = f.prefill(q, pool, sc, lens, cu, W, sinks, scale, cap)
                note("serving chain", check(*got, *f.ref_prefill(q, pool, sc, lens, cu, W, sinks, scale, cap), "%s chain prefill W=%s" % (fam, W)))
            else:
                q4 = q.view(B, Ts[0], Hq, D)
                got = f.decode(q4, pool, sc, lens, W, sinks, scale, cap)
                note("serving chain", check(*got, *f.ref_decode(q4, pool, sc, lens, W, sinks, scale, cap), "%s chain decode T=%d W=%s" % (fam, Ts[0], W)))


def test_zz_report_the_largest_error_over_bound(built, dev):
    """Prints what DESIGN 4.4.14 records; the siblings stayed below 0.4, and a ratio above 1 has failed its own test already."""
    for group, ratio in sorted(RATIOS.items()):
        print("largest O err / bound, %s: %.3f" % (group, ratio))
    assert all(r <= 1.0 for r in RATIOS.values())
