"""GPU: HOW MANY keys and WHICH keys every row of the sixteen bf16 paged attention entries sees, exactly, at every mask edge of
tests/paged_edge_cases.py (its docstring derives the two criteria; tests/test_paged_edge_cases.py shows on the CPU that the tables reach the
edges and that each modelled defect moves a count). D in {64, 128}; pools from paged_decode_reference.make_pool (shuffled placement, NaN -- the
e4m3 NaN byte -- in every page no live entry names and in the page the dead table entries point at), quantised by
paged_bf16_fp8_reference.quantize_pools; outputs pre-filled with O_FILL / L_FILL.

A. Counting: q = 0, K randn, V = 0.375. A row with n visible keys has LSE = ln n within 1 / (4 (n + 1)) and O = 0.375 bit for bit -- on the
   several-splits table too: the combine merges partials c n_s with factors exp2(0) = 1 and l = sum n_s, all exact, so no "one bf16 ulp"
   fallback was needed --; n = 0: O = 0, LSE = -inf; the rows of no sequence keep the fill. Sink entries again with a sink of 0 on every head:
   LSE = ln(n + 1) under the bound of n + 1, O within one bf16 ulp of c n / (n + 1). Soft-cap entries with (None, None) and with a scale and
   a cap of 2: the same bits. n comes from paged_edge_cases.visible, never from a kernel.
B. Identity: keys = the code of their position, q = 16 x the code of a target -- the row's lowest visible key, its highest, and on the
   several-splits table the last key of the first chunk and the first of the second: O = V[target] bit for bit, |LSE - score| <= 1e-5 score;
   with a sink equal to the score O = V[target] / 2 bit for bit and LSE = score + ln 2. Aimed at lo - 1 and hi + 1 (a key below the window; a
   later token's key, or a stale row past len) the rows must NOT return that key's V and must agree with the family's fp64 reference under the
   family's own check (test_gpu_paged_sink_attention.check over paged_softcap_reference, which is paged_sink_reference / paged_bf16_fp8_reference
   with scale = cap = None).
Every test prints the largest LSE err / bound of its table and the rows checked (pytest -s)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_all_entries as ae  # noqa: E402
import paged_edge_cases as ec  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import paged_softcap_reference as cr  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
O_FILL, L_FILL = sk.O_FILL, sk.L_FILL
NEG_INF = float("-inf")
FIRST, SPARE = 3, 5
bits, fbits = sk.bits, sk.fbits
NAMES = [e.name for e in ec.ENTRIES]
RATIOS = {}  # (table, sink) -> (largest LSE err / bound, rows)


def note(key, ratio, rows):
    old = RATIOS.get(key, (0.0, 0))
    RATIOS[key] = (max(old[0], ratio), old[1] + rows)


def run(e, q, pool, sc, lens, cu, W, sinks, floats, dev):
    """One call of entry e: (o, lse) on the CPU. sinks = None: no sink (NULL where the entry takes it, -inf per head else)."""
    kp, vp, bt = pool
    a = [t.to(dev) for t in (q, kp, vp, bt)] + [torch.tensor(list(lens), dtype=torch.int32, device=dev)]
    if cu is not None:
        a.append(torch.tensor(list(cu), dtype=torch.int32, device=dev))
    a += [s.to(dev) for s in sc]
    if e.window:
        a.append(ec.INT_MAX if W is None and not e.sink else W)
    if e.sink:
        if sinks is None and not (e.fp8 or e.anyg):
            sinks = sr.sinks_const(q.shape[-2], NEG_INF)
        a.append(None if sinks is None else sinks.to(dev))
    a += list(floats)
    o = torch.full(q.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(q.shape[:-1], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    getattr(ae.pkg(), e.name)(*a, o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def layout(case, Hq, D, rows_q):
    """(q, cu, seq): rows_q [R,Hq,D] in the order of paged_edge_cases.rows_of, as the entry wants them; seq: the slice of the packed rows of a
    sequence (the whole tensor for a decode)."""
    if case.T is not None:
        return rows_q.view(len(case.lens), case.T, Hq, D), None, None
    cu0 = ec.cu_of(case)
    q, cu = sr.pack(tuple(rows_q[cu0[b]:cu0[b + 1]] for b in range(len(case.Ts))), FIRST, SPARE)
    return q, cu, slice(cu[0], cu[-1])


def flat(case, o, lse, seq):
    """(o [R,Hq,D], lse [R,Hq]) in the order of rows_of; the rows of no sequence of a packed run must hold the fill."""
    if seq is None:
        return o.reshape(-1, *o.shape[-2:]), lse.reshape(-1, lse.shape[-1])
    for sl in (slice(0, seq.start), slice(seq.stop, None)):
        assert bool((bits(o[sl]) == O_FILL).all()) and bool((fbits(lse[sl]) == L_FILL).all()), case
    return o[seq], lse[seq]


def bf16_ulp(x):
    """One bf16 ulp at |x| (fp64 tensor, x != 0): 2^(floor(log2 |x|) - 7)."""
    return torch.exp2(torch.floor(torch.log2(x.abs())) - 7)


def check_counts(o, lse, n, sink, what):
    """The counting criterion on o [R,Hq,D], lse [R,Hq], n int64 [R]. Returns (largest LSE err / bound, rows x heads checked)."""
    live = n > 0
    assert bool((bits(o[~live]) == 0).all()) and bool((lse[~live] == NEG_INF).all()), what
    m = (n[live] + (1 if sink else 0)).double()
    want, bound = torch.log(m), 1.0 / (4.0 * (m + 1.0))
    ratio = ((lse[live].double() - want[:, None]).abs() / bound[:, None])
    worst = float(ratio.max()) if ratio.numel() else 0.0
    rows = int(live.sum()) * o.shape[1]
    print("%s: largest LSE err / bound %.4f over %d rows, n up to %d" % (what, worst, rows, int(n.max()) if n.numel() else 0))
    assert not bool(torch.isnan(ratio).any()) and worst <= 1.0, (what, worst)
    c = torch.tensor(ec.C_VALUE, dtype=BF)
    if not sink:
        assert bool((bits(o[live]) == int(bits(c))).all()), what
    else:
        expect = (ec.C_VALUE * n[live].double() / (n[live].double() + 1.0))[:, None, None]
        assert bool(((o[live].double() - expect).abs() <= bf16_ulp(expect)).all()), what
    return worst, rows


def count_case(e, D, case, dev):
    Hq = case.G * case.Hkv
    n = torch.tensor([v.n for v in ec.counts(case)], dtype=torch.int64)
    pool, sc = ec.count_pool(case.page, case.Nmax, case.lens, case.Hkv, D, e.fp8)
    q, cu, seq = layout(case, Hq, D, torch.zeros(len(n), Hq, D, dtype=BF))
    what = "%s D=%d %s page=%d T=%s G=%d W=%s" % (e.name, D, case.table, case.page, case.T, case.G, case.W)
    if case.table == "split":
        assert ec.plan_of(e, len(case.lens), case.T, Hq, case.Hkv, case.Nmax // case.page, case.page, D, case.W)[0] == case.S > 1, what
    elif case.table == "one":
        assert ec.plan_of(e, len(case.lens), case.T, Hq, case.Hkv, case.Nmax // case.page, case.page, D, case.W)[0] == 1, what
    for sink in ([False, True] if e.sink else [False]):
        first = None
        for floats in ec.softcap_configs(e, D):
            got = run(e, q, pool, sc, case.lens, cu, case.W, torch.zeros(Hq) if sink else None, floats, dev)
            if first is None:
                first = got
                o, lse = flat(case, *got, seq)
                note((case.table, sink), *check_counts(o, lse, n, sink, what + (" sink 0" if sink else "")))
            else:  # every score is 0 under any scale and cap: the same bits
                assert torch.equal(bits(got[0]), bits(first[0])) and torch.equal(fbits(got[1]), fbits(first[1])), (what, floats)


@pytest.mark.parametrize("D", ec.DS)
@pytest.mark.parametrize("name", [n for n in NAMES if "decode" in n])
def test_decode_with_one_split_counts_every_visible_key(built, dev, name, D):
    e = ae.BY_NAME[name]
    for case in ec.decode_one_cases(name, D):
        count_case(e, D, case, dev)


@pytest.mark.parametrize("D", ec.DS)
@pytest.mark.parametrize("name", [n for n in NAMES if "decode" in n])
def test_decode_with_several_splits_counts_every_visible_key(built, dev, name, D):
    e = ae.BY_NAME[name]
    for case in ec.decode_split_cases(name, D):
        count_case(e, D, case, dev)


@pytest.mark.parametrize("D", ec.DS)
@pytest.mark.parametrize("name", [n for n in NAMES if "prefill" in n])
def test_packed_prefill_counts_every_visible_key(built, dev, name, D):
    e = ae.BY_NAME[name]
    for case in ec.prefill_cases(name, D):
        count_case(e, D, case, dev)


# ---------------------------------------------------------------------------------------------------- B. identity

def subset(case, keep=8):
    """Every few lengths of a case, the last among them; a prefill case keeps its T_b with them."""
    idx = sorted(set(range(0, len(case.lens), max(1, len(case.lens) // keep))) | {len(case.lens) - 1})
    return case._replace(lens=tuple(case.lens[i] for i in idx), Ts=None if case.Ts is None else tuple(case.Ts[i] for i in idx))


def identity_case(e, D, case, dev):
    Hq = case.G * case.Hkv
    floats = ec.onehot_scale(e, D)
    x = floats[0] if floats else 1.0 / math.sqrt(D)
    score, margin = ec.onehot_score(case.Nmax, D, x)
    assert margin >= ec.ONEHOT_MARGIN
    vis = ec.counts(case)
    rows = ec.rows_of(case)
    pool, sc, V = ec.onehot_pool(case.page, case.Nmax, case.lens, case.Hkv, D, e.fp8)
    code = ec.codes(case.Nmax, D)
    what = "%s D=%d %s page=%d T=%s G=%d W=%s one-hot" % (e.name, D, case.table, case.page, case.T, case.G, case.W)

    def aimed(targets):
        """q whose row r is 16 x the code of targets[r] on every head (0 for a target of -1)."""
        t = torch.tensor(targets)
        rq = torch.where((t >= 0)[:, None], 16.0 * code[t.clamp(min=0)], torch.zeros(1, D))
        return layout(case, Hq, D, rq[:, None, :].expand(len(targets), Hq, D).to(BF).contiguous())

    variants = {"lo": [v.lo if v.n else -1 for v in vis], "hi": [v.hi if v.n else -1 for v in vis]}
    if case.table == "split":
        edge = [ec.base_of(min(max(case.lens[b], 0), case.Nmax), T, case.W, case.page) + case.C for b, t, T in rows]
        variants["last key of the first chunk"] = [j - 1 if v.n and v.lo <= j - 1 <= v.hi else -1 for j, v in zip(edge, vis)]
        variants["first key of the second chunk"] = [j if v.n and v.lo <= j <= v.hi else -1 for j, v in zip(edge, vis)]
        assert any(t >= 0 for t in variants["first key of the second chunk"]), what
    checked = 0
    for vname, targets in variants.items():
        t = torch.tensor(targets)
        hit = t >= 0
        q, cu, seq = aimed(targets)
        want = V[0][t.clamp(min=0)].to(BF)  # [R,D]; Hkv = 1
        for sink in ([False, True] if e.sink else [False]):
            sinks = torch.full((Hq,), score, dtype=torch.float32) if sink else None
            o, lse = flat(case, *run(e, q, pool, sc, case.lens, cu, case.W, sinks, floats, dev), seq)
            expect = (want.float() * (0.5 if sink else 1.0)).to(BF)[:, None, :].expand(-1, Hq, -1)
            assert torch.equal(bits(o[hit]), bits(expect[hit].contiguous())), (what, vname, sink)
            s = score + (math.log(2.0) if sink else 0.0)
            err = float((lse[hit].double() - s).abs().max())
            assert err <= 1e-5 * score, (what, vname, sink, err)
            checked += int(hit.sum()) * Hq
    # aimed at the hidden neighbours: not their V rows, and the family's fp64 reference under the family's check
    top = case.Nmax
    for vname, targets in (("lo - 1", [v.lo - 1 if v.n and v.lo >= 1 else -1 for v in vis]),
                           ("hi + 1", [v.hi + 1 if v.n and v.hi + 1 < top else -1 for v in vis])):
        t = torch.tensor(targets)
        hit = t >= 0
        if not bool(hit.any()):
            continue
        q, cu, seq = aimed(targets)
        got = run(e, q, pool, sc, case.lens, cu, case.W, None, floats, dev)
        o, lse = flat(case, *got, seq)
        hidden = V[0][t.clamp(min=0)].to(BF)[:, None, :].expand(-1, Hq, -1)
        same = (bits(o) == bits(hidden.contiguous())).all(dim=-1)
        assert not bool(same[hit].any()), (what, vname)
        kw = dict(ks=sc[0], vs=sc[1]) if e.fp8 else {}
        scale, cap = floats if floats else (None, None)
        if case.T is None:
            ro, rl, emul = cr.prefill(q, *pool, list(case.lens), cu, case.W, None, scale, cap, **kw)
            sk.check(got[0][seq], got[1][seq], ro[seq], rl[seq], emul[seq], what + " aimed at " + vname)
        else:
            sk.check(*got, *cr.decode(q, *pool, list(case.lens), case.W, None, scale, cap, **kw), what + " aimed at " + vname)
    print("%s: %d rows returned the V row of their target bit for bit" % (what, checked))
    assert checked


@pytest.mark.parametrize("D", ec.DS)
@pytest.mark.parametrize("name", NAMES)
def test_the_keys_at_both_edges_are_the_ones_a_row_sees(built, dev, name, D):
    e = ae.BY_NAME[name]
    for case in ec.onehot_cases(name, D):
        identity_case(e, D, subset(case), dev)


def test_zz_report_the_largest_lse_error_over_bound(built, dev):
    """Prints what paged_edge_cases.RATIOS_SEEN and DESIGN 4.4.15 record; a ratio above 1 has failed its own test already."""
    for (table, sink), (ratio, rows) in sorted(RATIOS.items()):
        print("largest LSE err / bound, table %s%s: %.4f over %d rows" % (table, ", sink 0" if sink else "", ratio, rows))
    assert all(r <= 1.0 for r, _ in RATIOS.values())
