"""GPU: the head-dim-256 entries of the bf16 paged path -- cuda_learn_notes_amd.kv_append_paged_varlen_d256_bf16,
fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16 and fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16 (csrc/*_d256_bf16.*;
DESIGN 4.4.16) -- against the references of their D = 64 / 128 siblings, which are generic in D: tests/paged_softcap_reference.py (fp64 and the
bf16 emulation) and tests/kv_append_bf16_reference.py. No new tolerance: O within paged_bf16_reference.o_bound of the emulation, LSE within
decode_reference.lse_tol per head, -inf LSE entries and zero rows exactly (test_gpu_paged_sink_attention.check). Beyond parity, bit for bit: a
packed sequence is its B = 1 call, sinks of -inf are sinks = None, a window past the cache is window = None, a scale of 1/16 is None, rows of no
sequence keep their fill; against the D = 128 entries on operands whose upper 128 dims are zero; and exact counts (q = 0, V = 1: O = 1, LSE =
ln of the visible keys) around the key steps and tile edges of the two kernels. Every parity case prints err / bound before it asserts
(pytest -s); the last test prints the largest per group."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_anyg_cases as ac  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import paged_edge_cases as ec  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import paged_softcap_reference as cr  # noqa: E402
import decode_reference as dr  # noqa: E402
import test_gpu_paged_bf16_fp8_attention as f8t  # noqa: E402
import test_gpu_paged_bf16_step as st  # noqa: E402  (the append problems and their checker)
import test_gpu_paged_sink_attention as sk  # noqa: E402
import prefill_varlen_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D = 256
O_FILL, L_FILL = sk.O_FILL, sk.L_FILL
NEG_INF = float("-inf")
bits, fbits, check, same = sk.bits, sk.fbits, sk.check, f8t.same
ROW_TILE, PREFILL_STEP, DECODE_STEP = 128, 64, 64  # the prefill's workgroup tile and key step, the decode's key step (4 waves x 16 keys)
DECODE_TG = [(1, 3), (8, 4), (2, 16), (3, 5), (8, 1)]  # one and two row tiles; 32 rows exactly twice
RATIOS = {}


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def prefill(q, pool, lens, cu, W, sinks, scale=None, cap=None, d128=False, dev="cuda"):
    c = pkg()
    fn = c.fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16 if d128 else c.fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16
    qd, kd, vd, bd = (t.to(dev) for t in (q, *pool))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:2], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    fn(qd, kd, vd, bd, sl, cd, W, None if sinks is None else sinks.to(dev), scale, cap, o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def decode(q, pool, lens, W, sinks, scale=None, cap=None, d128=False, dev="cuda"):
    c = pkg()
    name = "fa2_decode_paged_multi_window_sink_softcap_anyg_%sbf16" % ("" if d128 else "d256_")
    qd, kd, vd, bd = (t.to(dev) for t in (q, *pool))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:3], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    B, T, Hq, d = q.shape
    need = getattr(c, name + "_plan")(B, T, Hq, pool[0].shape[1], pool[2].shape[1], pool[0].shape[2], d, W)[2]  # sized from the entry's own plan
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    getattr(c, name)(qd, kd, vd, bd, sl, W, None if sinks is None else sinks.to(dev), scale, cap, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def plan(B, T, Hq, Hkv, max_pages, page, W):
    return pkg().fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, W)


# ---------------------------------------------------------------------------------------------------- 1. prefill parity

@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("G", [3, 8])
def test_prefill_rows_that_straddle_tiles(built, dev, G, page):
    """45 tokens x G = 135 or 360 rows: two or three 128-row tiles, the last one partial, tokens that straddle a tile edge at G = 3."""
    q, cu, lens, pool = cr.prefill_case(D, G, page)
    Hq = ac.P1_HKV * G
    assert q.shape[0] * G > ROW_TILE and (q.shape[0] * G) % ROW_TILE
    sinks = ac.sinks_for(Hq, 33)
    for W in (None, 33):
        for name, scale, cap in cr.configs(D):
            got = prefill(q, pool, lens, cu, W, sinks, scale, cap)
            note("prefill, one sequence, " + name, check(*got, *cr.prefill(q, *pool, lens, cu, W, sinks, scale, cap),
                                                         "prefill D=256 G=%d page=%d W=%s %s" % (G, page, W, name)))
            none = prefill(q, pool, lens, cu, W, None, scale, cap)
            note("prefill, one sequence, " + name, check(*none, *cr.prefill(q, *pool, lens, cu, W, None, scale, cap),
                                                         "prefill D=256 G=%d page=%d W=%s %s no sinks" % (G, page, W, name)))
        assert same(prefill(q, pool, lens, cu, W, sr.sinks_const(Hq, NEG_INF), cr.scale_for(D), cr.CAP), none), (G, page, W)


@pytest.mark.parametrize("G", [3, 8])
def test_packed_ragged_prefill_and_every_sequence_alone(built, dev, G):
    """T = 43, 0, 1, 26, 5: a sequence without a token, one whose 43 x 3 = 129 rows leave one row to a second tile, and -- with its length cut to
    20 -- one with len < T, whose first tokens see no key."""
    qs, lens, pool = cr.ragged_case(D, G)
    lens = list(lens)
    assert qs[1].shape[0] == 0 and qs[3].shape[0] == 26 and lens[3] > 20
    lens[3] = 20
    Hq, W = ac.P2_HKV * G, ac.P2_W
    q, cu = sr.pack(qs, 3, 5)
    seq = slice(cu[0], cu[-1])
    sinks = ac.sinks_for(Hq, W)
    for name, scale, cap in cr.configs(D):
        o, lse = prefill(q, pool, lens, cu, W, sinks, scale, cap)
        for sl in (slice(0, cu[0]), slice(cu[-1], None)):  # the rows of no sequence are untouched
            assert bool((bits(o[sl]) == O_FILL).all()) and bool((fbits(lse[sl]) == L_FILL).all())
        ro, rl, emul = cr.prefill(q, *pool, lens, cu, W, sinks, scale, cap)
        assert bool((rl[cu[3]:cu[3] + 6] == NEG_INF).all())  # len < T: the reference agrees that these rows see nothing
        note("prefill, packed, " + name, check(o[seq], lse[seq], ro[seq], rl[seq], emul[seq], "ragged prefill D=256 G=%d %s" % (G, name)))
    kp, vp, bt = pool
    for b, qb in enumerate(qs):  # every sequence alone, B = 1: the packed run's bits (o, lse: the last config's, scale + cap)
        t = qb.shape[0]
        q1 = torch.cat((qb, torch.full((1,) + tuple(qb.shape[1:]), 2.0 ** 100, dtype=BF)))
        o1, l1 = prefill(q1, (kp, vp, bt[b:b + 1].contiguous()), [lens[b]], [0, t], W, sinks, scale, cap)
        assert torch.equal(bits(o1[:t]), bits(o[cu[b]:cu[b + 1]])) and torch.equal(fbits(l1[:t]), fbits(lse[cu[b]:cu[b + 1]])), (G, b)
        assert bool((bits(o1[t:]) == O_FILL).all())


# ---------------------------------------------------------------------------------------------------- 2. decode parity

@pytest.mark.parametrize("TG", DECODE_TG, ids=lambda tg: "T%dxG%d" % tg)
def test_decode_one_split(built, dev, TG):
    T, G = TG
    q, lens, pool = cr.decode_one_case(T, G, D)  # lens 0, 1, 17, 100, 257 at page 16
    Hq = ac.D3_HKV * G
    sinks = ac.sinks_for(Hq, 33)
    for W in (None, 33):
        assert plan(len(lens), T, Hq, ac.D3_HKV, ac.D3_NMAX // ac.PAGE, ac.PAGE, W)[0] == 1
        for name, scale, cap in cr.configs(D):
            got = decode(q, pool, lens, W, sinks, scale, cap)
            note("decode, one split, " + name, check(*got, *cr.decode(q, *pool, lens, W, sinks, scale, cap),
                                                     "decode S=1 D=256 T=%d G=%d W=%s %s" % (T, G, W, name)))
        none = decode(q, pool, lens, W, None, cr.scale_for(D), cr.CAP)
        note("decode, one split, scale+cap", check(*none, *cr.decode(q, *pool, lens, W, None, cr.scale_for(D), cr.CAP),
                                                   "decode S=1 D=256 T=%d G=%d W=%s no sinks" % (T, G, W)))
        assert bool((none[0][0] == 0).all()) and bool((none[1][0] == NEG_INF).all())  # len 0 sees no key
        assert same(decode(q, pool, lens, W, sr.sinks_const(Hq, NEG_INF), cr.scale_for(D), cr.CAP), none), (T, G, W)


@pytest.mark.parametrize("TG", [(3, 5), (8, 4)], ids=lambda tg: "T%dxG%d" % tg)
def test_decode_several_splits(built, dev, TG):
    """A table of 4096 keys: 16 splits without a window, 4 with W = 1000. Which splits of a sequence hold keys:
      len 4096, W = 1000  the splits start at base = align_down(4096 - T - 1000 + 1, 64) = 3072, not at 0: every one of the 4 holds keys, and the
                          up to 63 keys between base and the first query's lower edge are hidden from every row by the mask
      len 4096, no window all 16 splits hold keys
      len 1000, no window the first 4 of the 16 splits hold keys, the other 12 write nothing and the combine skips them
      len 1000, W = 1000  base = 0: the keys lie in the leading splits, the trailing ones are empty
    A LEADING split without a row of its own cannot arise under this plan: the splits divide the span from base on, base is at most U - 1 = 63
    keys below the first query's lower edge, and a chunk is at least 256 keys when there is more than one, so split 0 always holds a key the
    first query sees; and query t's lower edge is only t <= 7 keys above it. What does arise is a split whose keys a LATER row does not need
    and an empty trailing split, both covered here; the mixed batch below puts a long and a short sequence into one launch, so that workgroups
    with and without keys and rows with 4 and with 1 live partial meet in one combine."""
    T, G = TG
    for W in (None, 1000):
        S = plan(1, T, G, 1, ac.D4_NMAX // ac.PAGE, ac.PAGE, W)[0]
        assert S >= 3, (W, S)
        for n in (4096, 1000):
            q, lens, pool = cr.decode_split_case(T, G, D, n)
            sinks = ac.sinks_for(G, n if W is None else min(W, n))
            for name, scale, cap in cr.configs(D):
                got = decode(q, pool, lens, W, sinks, scale, cap)
                note("decode, several splits, " + name, check(*got, *cr.decode(q, *pool, lens, W, sinks, scale, cap),
                                                              "decode S=%d D=256 T=%d G=%d W=%s len=%d %s" % (S, T, G, W, n, name)))
            none = decode(q, pool, lens, W, None, None, cr.CAP)
            assert same(decode(q, pool, lens, W, sr.sinks_const(G, NEG_INF), None, cr.CAP), none), (T, G, W, n)
    # one launch, three sequences: the whole table, 300 keys (one live split) and none at all
    lens = [4096, 300, 0]
    g = torch.Generator().manual_seed(77 + T + G)
    k, v = (torch.randn(3, 1, ac.D4_NMAX, D, generator=g).to(BF) for _ in range(2))
    q = (torch.randn(3, T, G, D, generator=g) * cr.Q_MUL).to(BF)
    pool = pr.make_pool(k, v, ac.PAGE, lens, seed=5)
    sinks = ac.sinks_for(G, 300)
    for W in (None, 1000):
        assert plan(3, T, G, 1, ac.D4_NMAX // ac.PAGE, ac.PAGE, W)[0] >= 3
        got = decode(q, pool, lens, W, sinks, cr.scale_for(D), cr.CAP)
        note("decode, several splits, scale+cap", check(*got, *cr.decode(q, *pool, lens, W, sinks, cr.scale_for(D), cr.CAP),
                                                        "decode mixed batch D=256 T=%d G=%d W=%s" % (T, G, W)))
        assert bool((got[0][2] == 0).all()) and bool((got[1][2] == NEG_INF).all())  # len 0: no split holds a key, the combine still writes the row


# ---------------------------------------------------------------------------------------------------- 3. bit equalities

def test_a_window_past_the_cache_is_none_and_a_scale_of_one_sixteenth_is_none(built, dev):
    """256^-1/2 = 0.0625 is a float: (float)(0.0625 log2 e) and (float)(log2 e / 16) are one number."""
    q, cu, lens, pool = cr.prefill_case(D, 3, 16)
    sinks = ac.sinks_for(ac.P1_HKV * 3, 33)
    for cap in (None, cr.CAP):
        base = prefill(q, pool, lens, cu, None, sinks, None, cap)
        assert same(prefill(q, pool, lens, cu, 33, sinks, 0.0625, cap), prefill(q, pool, lens, cu, 33, sinks, None, cap)), cap
        assert same(prefill(q, pool, lens, cu, ac.P1_NMAX, sinks, None, cap), base) and same(prefill(q, pool, lens, cu, 10 ** 6, sinks, None, cap), base)
    q, lens, pool = cr.decode_one_case(8, 4, D)
    sinks = ac.sinks_for(ac.D3_HKV * 4, 33)
    for cap in (None, cr.CAP):
        base = decode(q, pool, lens, None, sinks, None, cap)
        assert same(decode(q, pool, lens, 33, sinks, 0.0625, cap), decode(q, pool, lens, 33, sinks, None, cap)), cap
        assert same(decode(q, pool, lens, ac.D3_NMAX, sinks, None, cap), base), cap
    q, lens, pool = cr.decode_split_case(3, 5, D, 4096)  # several splits: a window of the whole table plans as no window does
    assert same(decode(q, pool, lens, 4096, None, None, cr.CAP), decode(q, pool, lens, None, None, None, cr.CAP))


# ---------------------------------------------------------------------------------------------------- 4. against the D = 128 entries

def _upper_half_zero(t):
    t = t.clone()
    t[..., 128:] = 0
    return t


def _check_halves(got, want, emul_bound, what):
    """got: the D = 256 entry's (o, lse); want: the D = 128 entry's on the lower halves. o_bound is formed from the D = 128 output as both the
    emulation and the reference would be: the bf16 rounding of O, which is what separates two correct kernels."""
    o, lse = got
    o1, l1 = want
    assert bool((bits(o[..., 128:]) == 0).all()), what  # exactly +0: V's upper dims are zero
    fin = torch.isfinite(l1)
    assert torch.equal(torch.isfinite(lse), fin), what
    eo = (o[..., :128].double() - o1.double()).abs().max().item()
    worst = 0.0
    for h in range(l1.shape[-1]):  # head by head, as check() does: a head whose sink is 1e30 has an LSE of that size
        f = fin[..., h]
        if bool(f.any()):
            el, bl = (lse[..., h].double()[f] - l1[..., h].double()[f]).abs().max().item(), dr.lse_tol(l1[..., h].double())
            worst = max(worst, el / bl)
            assert el <= bl, (what, h, el, bl)
    print("%s: O err %.3e / bound %.3e = %.4f   LSE err / tol %.4f" % (what, eo, emul_bound, eo / emul_bound, worst))
    assert eo <= emul_bound, (what, eo, emul_bound)
    return eo / emul_bound


def test_prefill_and_decode_agree_with_the_d128_entries_on_zero_upper_dims(built, dev):
    x = 128 ** -0.5
    for G, cap in ((3, None), (8, cr.CAP)):
        q, cu, lens, (kp, vp, bt) = cr.prefill_case(D, G, 16)
        q, kp, vp = _upper_half_zero(q), _upper_half_zero(kp), _upper_half_zero(vp)
        sinks = ac.sinks_for(ac.P1_HKV * G, 33)
        lo = tuple(t[..., :128].contiguous() for t in (q, kp, vp))
        ro, _, emul = cr.prefill(lo[0], lo[1], lo[2], bt, lens, cu, 33, sinks, x, cap)
        got = prefill(q, (kp, vp, bt), lens, cu, 33, sinks, x, cap)
        want = prefill(lo[0], (lo[1], lo[2], bt), lens, cu, 33, sinks, x, cap, d128=True)
        note("prefill, against D = 128", _check_halves(got, want, br.o_bound(emul, ro), "prefill D=256 vs D=128 G=%d cap=%s" % (G, cap)))
    for (T, G), cap in (((3, 5), None), ((8, 4), cr.CAP)):
        q, lens, (kp, vp, bt) = cr.decode_one_case(T, G, D)
        q, kp, vp = _upper_half_zero(q), _upper_half_zero(kp), _upper_half_zero(vp)
        sinks = ac.sinks_for(ac.D3_HKV * G, 33)
        lo = tuple(t[..., :128].contiguous() for t in (q, kp, vp))
        ro, _, emul = cr.decode(lo[0], lo[1], lo[2], bt, lens, 33, sinks, x, cap)
        fin = torch.isfinite(ro)
        got = decode(q, (kp, vp, bt), lens, 33, sinks, x, cap)
        want = decode(lo[0], (lo[1], lo[2], bt), lens, 33, sinks, x, cap, d128=True)
        note("decode, against D = 128", _check_halves(got, want, br.o_bound(emul[fin], ro[fin]), "decode D=256 vs D=128 T=%d G=%d cap=%s" % (T, G, cap)))


# ---------------------------------------------------------------------------------------------------- 5. exact counts

def _count_pool(page, Nmax, lens, Hkv):
    g = torch.Generator().manual_seed(page + Nmax)
    k = torch.randn(1, Hkv, Nmax, D, generator=g).to(BF).expand(len(lens), Hkv, Nmax, D)
    v = torch.ones(1, Hkv, Nmax, D, dtype=BF).expand(len(lens), Hkv, Nmax, D)
    return pr.make_pool(k, v, page, list(lens), seed=len(lens))


def _check_counts(o, lse, lens, T, W, Nmax, rows_of, what):
    worst = 0.0
    for b, n_b in enumerate(lens):
        for t in range(T[b] if isinstance(T, list) else T):
            n = ec.visible(n_b, T[b] if isinstance(T, list) else T, t, W, Nmax).n
            ob, lb = rows_of(o, lse, b, t)
            if n == 0:
                assert bool((bits(ob) == 0).all()) and bool((lb == NEG_INF).all()), (what, b, t)
                continue
            assert bool((ob == 1).all()), (what, b, t, n)  # q = 0: every weight is 1 / n, V = 1, and the fp32 sum of n weights times 1 / l is 1
            err, tol = (lb.double() - math.log(n)).abs().max().item(), ec.lse_tol_at(n)
            worst = max(worst, err / tol)
            assert err <= tol, (what, b, t, n, err, tol)
    print("%s: LSE = ln(visible keys) within %.4f of the tolerance" % (what, worst))


def test_exact_counts_around_the_key_steps_and_tile_edges(built, dev):
    """q = 0 and V = 1: O is exactly 1 and LSE = ln of the keys the row sees. Decode lengths n, n +- 1 around the 16-key block of a wave, the
    64-key step and two of them, with and without a window; prefill lengths around the 64-key step with T G around the 128-row tile."""
    Nmax, page, Hkv, G, T = 272, 16, 2, 4, 8
    lens = sorted({n + d for n in (16, 64, 128) for d in (-1, 0, 1)} | {8, 257})
    pool = _count_pool(page, Nmax, tuple(lens), Hkv)
    q = torch.zeros(len(lens), T, Hkv * G, D, dtype=BF)
    for W in (None, 17, 64, 65):
        assert plan(len(lens), T, Hkv * G, Hkv, Nmax // page, page, W)[0] == 1
        for cap in (None, 50.0):
            o, lse = decode(q, pool, lens, W, None, None, cap)
            _check_counts(o, lse, lens, T, W, Nmax, lambda o, lse, b, t: (o[b, t], lse[b, t]), "decode counts W=%s cap=%s" % (W, cap))
    G = 3
    Ts = [43, 42, 44, 1]  # 129, 126 and 132 rows: the 128-row tile's edge inside a token, before it and after it
    ctx = [63, 64, 65, 0]
    lens = [c + t for c, t in zip(ctx, Ts)]
    pool = _count_pool(page, Nmax, tuple(lens), Hkv)
    cu = [0]
    for t in Ts:
        cu.append(cu[-1] + t)
    q = torch.zeros(cu[-1], Hkv * G, D, dtype=BF)
    for W in (None, 17, 64, 65):
        for cap in (None, 50.0):
            o, lse = prefill(q, pool, lens, cu, W, None, None, cap)
            _check_counts(o, lse, lens, Ts, W, Nmax, lambda o, lse, b, t: (o[cu[b] + t], lse[cu[b] + t]), "prefill counts W=%s cap=%s" % (W, cap))


# ---------------------------------------------------------------------------------------------------- 6. append, and the chain

def run_append(k_new, v_new, kp, vp, bt, lens, cu, q=None, table=None, rope="none", dev="cuda"):
    knd, vnd, kd, vd, bd = (t.to(dev) for t in (k_new, v_new, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    qd = qo = td = None
    if q is not None:
        qd = q.to(dev)
        qo = torch.full(qd.shape, st.Q_FILL, dtype=torch.int16, device=dev).view(BF)
    if table is not None:
        td = table.to(dev)
    pkg().kv_append_paged_varlen_d256_bf16(knd, vnd, kd, vd, bd, sl, cd, qd, qo, td, rope)
    torch.cuda.synchronize()
    assert torch.equal(bits(knd.cpu()), bits(k_new)) and torch.equal(bits(vnd.cpu()), bits(v_new))
    return kd.cpu(), vd.cpu(), (qo.cpu() if qo is not None else None)


def _ragged_append_case():
    """The first ragged case of prefill_varlen_reference.CASES with more than one sequence whose runs cross a page edge (st.lengths puts the runs
    of the middle sequences on the last row of a page)."""
    for ci, (geom, T) in enumerate(vr.CASES):
        if len(T) >= 3 and len(set(T)) > 1 and any(t > 1 for t in T[1:-1]):
            return ci
    raise AssertionError("no ragged case")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_append_against_the_reference(built, dev, mode):
    """Mode 0: every row bit for bit. Modes 1 and 2: V bit for bit, K and q_out within the reference's own bound (one rounding of an fp32
    rotation), as at D = 64 and 128; the half-split partner of column i is i + 128."""
    ci = _ragged_append_case()
    geom, T = vr.CASES[ci]
    page = geom[2]
    k_new, v_new, q, cu, k, v = st.problem(ci, D)
    lens = st.lengths(geom, T)
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=ci)
    what = "append D=256 %s %s" % (st.CASE_IDS[ci], st.MODE_NAMES[mode])
    if mode == 0:
        gk, gv, _ = run_append(k_new, v_new, kp, vp, bt, lens, cu)
        rows, dead = st.check_reference(gk, gv, None, k_new, v_new, kp, vp, bt, lens, cu, None, None, 0, page, what)
    else:
        table = st.random_table(page * geom[3], D)
        gk, gv, qo = run_append(k_new, v_new, kp, vp, bt, lens, cu, q, table, st.MODE_NAMES[mode])
        rows, dead = st.check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q, table, mode, page, what)
    assert len(rows) == sum(T) and not dead and not torch.equal(bits(gk), bits(kp))
    assert any(pos % page == page - 1 for (_, _, pos, *_) in rows) and any(pos % page == 0 for (_, _, pos, *_) in rows)  # a page edge is crossed


def test_gemma2_9b_chain_append_prefill_decode(built, dev):
    """Gemma-2-9B's numbers: Hq 16, Hkv 8, D 256, cap 50, scale 1 / 16 = 256^-1/2 (query_pre_attn_scalar 256), W 4096 on a cache shorter than W,
    half-split RoPE. A prompt of 70 tokens is appended and attended to (prefill), then 3 more tokens are appended and attended to (decode); the
    reference attends over the pools the reference append fills. The pools the kernels fill differ from those by at most the append's rounding,
    so the attention reference is run on the kernel's own pools: each stage is held to its own bound."""
    import cuda_learn_notes_amd as c
    Hq, Hkv, page, mp, cap, scale, W = 16, 8, 16, 6, 50.0, 1.0 / 16, 4096
    g = torch.Generator().manual_seed(9)
    Tp, Td = 70, 3
    kp = torch.zeros(mp + 1, Hkv, page, D, dtype=BF)
    vp = torch.zeros_like(kp)
    bt = torch.randperm(mp, generator=g).to(torch.int32)[None].contiguous()
    table = c.kv_append_rope_table(page * mp, D)
    sinks = None
    for T, len_after, kind in ((Tp, Tp, "prefill"), (Td, Tp + Td, "decode")):
        k_new, v_new, q = ((torch.randn(T, H, D, generator=g)).to(BF) for H in (Hkv, Hkv, Hq))
        cu, lens = [0, T], [len_after]
        gk, gv, qo = run_append(k_new, v_new, kp, vp, bt, lens, cu, q, table, "half")
        st.check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q, table, 1, page, "chain append before the %s" % kind)
        kp, vp = gk, gv
        if kind == "prefill":
            got = prefill(qo, (kp, vp, bt), lens, cu, W, sinks, scale, cap)
            ref = cr.prefill(qo, kp, vp, bt, lens, cu, W, sinks, scale, cap)
        else:
            got = decode(qo[None].contiguous(), (kp, vp, bt), lens, W, sinks, scale, cap)
            ref = cr.decode(qo[None].contiguous(), kp, vp, bt, lens, W, sinks, scale, cap)
        note("chain, " + kind, check(*got, *ref, "Gemma-2-9B chain %s" % kind))


# ---------------------------------------------------------------------------------------------------- 7. bad arguments, summary

def test_python_entries_refuse_other_head_dims_and_too_many_rows(built, dev):
    c = pkg()
    b = lambda *s: torch.zeros(*s, dtype=BF, device="cuda")  # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")  # noqa: E731
    with pytest.raises(RuntimeError, match=r"head dim 128 not supported \(256\)"):
        c.fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16(b(4, 4, 128), b(3, 2, 16, 128), b(3, 2, 16, 128), i(1, 2), i(1), i(2), None,
                                                                      None, None, None, b(4, 4, 128))
    with pytest.raises(RuntimeError, match=r"head dim 128 not supported \(256\)"):
        c.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(b(1, 2, 4, 128), b(3, 2, 16, 128), b(3, 2, 16, 128), i(1, 2), i(1), None, None,
                                                                    None, None, b(1, 2, 4, 128))
    with pytest.raises(RuntimeError, match=r"head dim 64 not supported \(256\)"):
        c.kv_append_paged_varlen_d256_bf16(b(4, 2, 64), b(4, 2, 64), b(3, 2, 16, 64), b(3, 2, 16, 64), i(1, 2), i(1), i(2))
    with pytest.raises(RuntimeError, match=r"T 5 x group size 7 = 35 query rows"):
        c.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(b(1, 5, 7, 256), b(3, 1, 16, 256), b(3, 1, 16, 256), i(1, 2), i(1), None, None,
                                                                    None, None, b(1, 5, 7, 256))


def test_zz_summary_of_error_over_bound(built, dev):
    """The RATIOS table: the largest O err / bound of every group of parity cases of this file. Not an assertion of its own --
    every case asserted err <= bound where it ran."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-44s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
