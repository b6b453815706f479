"""GPU: multi-head latent attention over a paged latent cache -- cuda_learn_notes_amd.fa2_decode_paged_mla_bf16 and kv_append_paged_mla_bf16
(csrc/*_mla_bf16.*) -- against tests/paged_mla_reference.py (fp64 and the bf16 emulation, anchored to the existing reference by
tests/test_paged_mla_surface.py) and tests/kv_append_bf16_reference.py on the 64 rotary dims. No new tolerance: O within
paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol per head, -inf LSE entries and zero rows exactly
(test_gpu_paged_sink_attention.check). Beyond parity: exact counts (q = 0, value dims 1: O = 1, LSE = ln of the visible keys) around every key
block, step and chunk edge, the rotary dims inside the score and outside the value, and bit equalities -- a sequence alone, guard bands, two
calls, a captured graph. Every parity case prints err / bound before it asserts (pytest -s); the last test prints the largest per group.

Largest err / bound of O seen on an MI355X: see DESIGN 4.4.17 and profiles/r27_paged_mla_tests.log."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import kv_append_bf16_reference as ar  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_edge_cases as ec  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DC, DR, DK, SCALE = ml.DC, ml.DR, ml.DK, ml.SCALE
O_FILL, L_FILL, Q_FILL = sk.O_FILL, sk.L_FILL, 0x3C5A
NEG_INF = float("-inf")
bits, fbits, check = sk.bits, sk.fbits, sk.check
RATIOS = {}


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def plan(B, T, Hq, pool):
    return pkg().fa2_decode_paged_mla_bf16_plan(B, T, Hq, pool[1].shape[1], pool[0].shape[1])


def decode(q, pool, lens, scale=SCALE, dev="cuda"):
    """(o, lse) on the CPU; the workspace is sized from the entry's own plan."""
    c = pkg()
    qd, pd, bd = (t.to(dev) for t in (q, *pool))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    B, T, Hq, _ = q.shape
    o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    ws = torch.empty(max(plan(B, T, Hq, pool)[2], 16), dtype=torch.uint8, device=dev)
    c.fa2_decode_paged_mla_bf16(qd, pd, bd, sl, scale, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def same(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(fbits(a[1]), fbits(b[1]))


# ---------------------------------------------------------------------------------------------------- 1. one split

@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("TH", ml.ONE_TH, ids=lambda th: "T%dxHq%d" % th)
def test_decode_one_split(built, dev, TH, page):
    """Lengths 0, 1, 17, 63, 64, 65, 100, 257 (at T = 8: 0, 1, 2, 5, 7, 8, 100, 257, lengths below T whose first tokens see no key); R = T Hq
    from 1 row to four row groups of 64, 17 and 65 rows leaving one row to a second tile resp. a second row group."""
    T, Hq = TH
    q, lens, pool = ml.one_case(T, Hq, page)
    assert plan(len(lens), T, Hq, pool)[0] == 1
    got = decode(q, pool, lens)
    ro, rl, emul = ml.decode(q, *pool, lens, SCALE)
    assert bool((rl[0] == NEG_INF).all())
    if T == 8:
        assert bool((rl[3, :3] == NEG_INF).all()) and bool(torch.isfinite(rl[3, 3:]).all())  # len 5 < T
    note("decode, one split", check(*got, ro, rl, emul, "mla S=1 T=%d Hq=%d page=%d" % (T, Hq, page)))


# ---------------------------------------------------------------------------------------------------- 2. several splits

@pytest.mark.parametrize("TH", ml.SPLIT_TH, ids=lambda th: "T%dxHq%d" % th)
def test_decode_several_splits(built, dev, TH):
    """B = 5 at page 16 with 64 table entries: 4 splits of 256 keys. Lengths 1000 (every split), 300 and 257 (two, the second with 44 keys and
    with one), 100 (one) and 0 (none: the combine still writes the row). The same sequences on a table cut to 16 pages plan one split: where the
    sequence fits, the two results agree within the bound."""
    T, Hq = TH
    q, lens, pool = ml.split_case(T, Hq)
    S, C, _ = plan(len(lens), T, Hq, pool)
    assert S > 1 and (S, C) == (4, 256), (S, C)
    got = decode(q, pool, lens)
    ro, rl, emul = ml.decode(q, *pool, lens, SCALE)
    note("decode, several splits", check(*got, ro, rl, emul, "mla S=%d T=%d Hq=%d" % (S, T, Hq)))
    assert bool((got[0][4] == 0).all()) and bool((got[1][4] == NEG_INF).all())
    cut = (pool[0], pool[1][:, :16].contiguous())
    clipped = [min(n, 256) for n in lens]
    assert plan(len(lens), T, Hq, cut)[0] == 1
    one = decode(q, cut, clipped)
    r1 = ml.decode(q, *cut, clipped, SCALE)
    note("decode, one split", check(*one, *r1, "mla S=1 on the cut table T=%d Hq=%d" % (T, Hq)))
    fits = [b for b, n in enumerate(lens) if n <= 256]
    assert fits == [3, 4]
    bound = br.o_bound(emul[fits], ro[fits])
    eo = float((got[0][fits].double() - one[0][fits].double()).abs().max())
    el = float((got[1][3].double() - one[1][3].double()).abs().max())
    print("mla S=%d against S=1 T=%d Hq=%d: O diff %.3e / bound %.3e = %.4f, LSE diff %.3e" % (S, T, Hq, eo, bound, eo / bound, el))
    assert eo <= bound and el <= dr.lse_tol(rl[3]) and same((one[0][4], one[1][4]), (got[0][4], got[1][4]))


# ---------------------------------------------------------------------------------------------------- 2b. a scale that is not the data's

@pytest.mark.parametrize("scale", ml.OTHER_SCALES, ids=["yarn", "quarter"])
@pytest.mark.parametrize("case", ml.SCALE_TH, ids=lambda c: "T%dxHq%d%s" % (c[0], c[1], "-split" if c[2] else ""))
def test_decode_at_a_scale_that_is_not_the_datas(built, dev, case, scale):
    """The one-split case at (3, 5) and the several-splits case at (2, 40) at V3's YaRN scale and at SCALE / 4, q x Q_MULT so that the softmax is
    far from flat: the reference at SCALE is more than 20 x o_bound away (proven without a GPU by tests/test_paged_mla_surface.py)."""
    T, Hq, split = case
    q, lens, pool, ref, ref0 = ml.scale_case(T, Hq, split, scale)
    S = plan(len(lens), T, Hq, pool)[0]
    assert (S > 1) == split
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla scale %.5f T=%d Hq=%d S=%d: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, T, Hq, S, diff, need))
    assert diff > need
    note("decode, another scale", check(*decode(q, pool, lens, scale=scale), *ref, "mla scale=%.5f S=%d T=%d Hq=%d" % (scale, S, T, Hq)))


def _graph_replays_eager(call, B, T, Hq, need):
    """call(o, lse, ws) eager, then captured in a graph and replayed on fresh buffers: (eager o, lse on the CPU), bit for bit the replay's."""
    def buffers():
        return (torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device="cuda").view(BF),
                torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device="cuda").view(torch.float32), torch.empty(need, dtype=torch.uint8, device="cuda"))

    eager = buffers()
    call(*eager)
    torch.cuda.synchronize()
    o, lse = eager[0].cpu(), eager[1].cpu()
    bufs = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(*bufs)
    torch.cuda.synchronize()
    assert bool((bits(bufs[0].cpu()) == O_FILL).all())  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(bufs[0].cpu()), bits(o)) and torch.equal(fbits(bufs[1].cpu()), fbits(lse))
    return o, lse


def test_decode_at_the_yarn_scale_through_a_captured_graph(built, dev):
    """The several-splits case at (2, 40) at YARN: the stream kernel and the combine captured and replayed, bit for bit the eager result."""
    c = pkg()
    T, Hq = 2, 40
    q, lens, pool, ref, _ = ml.scale_case(T, Hq, True, ml.YARN)
    B = len(lens)
    S, _, need = plan(B, T, Hq, pool)
    assert S > 1
    fixed = (q.to("cuda"), pool[0].to("cuda"), pool[1].to("cuda"), torch.tensor(lens, dtype=torch.int32, device="cuda"))
    o, lse = _graph_replays_eager(lambda o, lse, ws: c.fa2_decode_paged_mla_bf16(*fixed, ml.YARN, o, lse, ws), B, T, Hq, need)
    note("decode, another scale", check(o, lse, *ref, "mla scale=YARN eager, then a captured graph S=%d" % S))


# ---------------------------------------------------------------------------------------------------- 3. exact counts

@pytest.mark.parametrize("max_pages", [20, 64], ids=["one-split", "several-splits"])
@pytest.mark.parametrize("TH", [(1, 16), (3, 5)], ids=lambda th: "T%dxHq%d" % th)
def test_exact_counts(built, dev, TH, max_pages):
    """q = 0, value dims = 1, rotary dims random: every weight of a row is 1 / n, so O is exactly 1 and LSE = ln n, n = the keys the row sees:
    lengths around the 16-key block, the 64-key step and the 256-key chunk."""
    T, Hq = TH
    lens, page = ml.COUNT_N, 16
    g = torch.Generator().manual_seed(max_pages)
    dense = torch.ones(1, max_pages * page, DK)
    dense[..., DC:] = torch.randn(1, max_pages * page, DR, generator=g)
    pool = ml.make_pool(dense.to(BF).expand(len(lens), -1, -1), page, lens, seed=3)
    S = plan(len(lens), T, Hq, pool)[0]
    assert (S == 1) == (max_pages == 20), S
    q = torch.zeros(len(lens), T, Hq, DK, dtype=BF)
    o, lse = decode(q, pool, lens)
    worst = 0.0
    for b, n_b in enumerate(lens):
        for t in range(T):
            n = max(n_b - (T - 1 - t), 0)
            if n == 0:
                assert bool((bits(o[b, t]) == 0).all()) and bool((lse[b, t] == NEG_INF).all()), (b, t)
                continue
            assert bool((o[b, t] == 1).all()), (b, t, n)
            err, tol = (lse[b, t].double() - math.log(n)).abs().max().item(), ec.lse_tol_at(n)
            worst = max(worst, err / tol)
            assert err <= tol, (b, t, n, err, tol)
    print("mla counts T=%d Hq=%d S=%d: LSE = ln(visible keys) within %.4f of the tolerance" % (T, Hq, S, worst))


# ---------------------------------------------------------------------------------------------------- 4, 5. the rotary dims

def test_key_only_dims_stay_out_of_the_value(built, dev):
    """q_pe = 0: the rotary dims of the pool meet zeros in the score and must not be read as value at all: the same bits whether they hold 0 or
    +-2^60."""
    for (T, Hq), case in (((3, 5), ml.one_case(3, 5, 16)), ((2, 40), ml.split_case(2, 40))):
        q, lens, (pool, bt) = case
        q = q.clone()
        q[..., DC:] = 0
        zero, big = pool.clone(), pool.clone()
        zero[..., DC:] = 0
        big[..., DC:] = 2.0 ** 60
        big[..., DC::2] = -2.0 ** 60
        a, b = decode(q, (zero, bt), lens), decode(q, (big, bt), lens)
        assert same(a, b), (T, Hq)
        note("decode, q_pe = 0", check(*a, *ml.decode(q, zero, bt, lens, SCALE), "mla q_pe=0 T=%d Hq=%d" % (T, Hq)))


def test_rotary_dims_reach_the_scores(built, dev):
    """q_nope = 0 and random rotary dims 32 times the usual size in q and in the pool: the scores (standard deviation about 3) are the rotary
    dims' alone, the softmax is far from uniform, and the result is the reference's."""
    for (T, Hq), case in (((3, 5), ml.one_case(3, 5, 16)), ((2, 40), ml.split_case(2, 40))):
        q, lens, (pool, bt) = case
        q = q.clone()
        q[..., :DC] = 0
        q[..., DC:] = (q[..., DC:].float() * 32).to(BF)
        pool = pool.clone()
        pool[..., DC:] = (pool[..., DC:].float() * 32).to(BF)  # 2^100 stays finite in bf16
        got = decode(q, (pool, bt), lens)
        ro, rl, emul = ml.decode(q, pool, bt, lens, SCALE)
        flat = ml.decode(q * 0, pool, bt, lens, SCALE)[0]
        assert float((ro - flat).abs().max()) > 20 * br.o_bound(emul, ro)  # the uniform average is far outside the bound
        note("decode, q_nope = 0", check(*got, ro, rl, emul, "mla q_nope=0 T=%d Hq=%d" % (T, Hq)))


# ---------------------------------------------------------------------------------------------------- 6. bit equalities

def test_a_sequence_alone_guard_bands_and_two_calls(built, dev):
    c = pkg()
    T, Hq, page = 1, 16, 16
    q, lens, (pool, bt) = ml.one_case(T, Hq, page)
    B = len(lens)
    base = decode(q, (pool, bt), lens)
    assert same(decode(q, (pool, bt), lens), base)  # two calls
    for b in range(B):  # alone: B = 1 with its table row (the plan is one split for either B)
        one = decode(q[b:b + 1].contiguous(), (pool, bt[b:b + 1].contiguous()), lens[b:b + 1])
        assert same(one, (base[0][b:b + 1], base[1][b:b + 1])), b
    # guard bands: the region passed lies inside larger tensors
    dev_ = "cuda"
    big_o = torch.full((B + 2, T, Hq, DC), O_FILL, dtype=torch.int16, device=dev_).view(BF)
    big_l = torch.full((B + 2, T, Hq), L_FILL, dtype=torch.int32, device=dev_).view(torch.float32)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev_)
    c.fa2_decode_paged_mla_bf16(q.to(dev_), pool.to(dev_), bt.to(dev_), sl, SCALE, big_o[1:B + 1], big_l[1:B + 1])
    torch.cuda.synchronize()
    big_o, big_l = big_o.cpu(), big_l.cpu()
    assert same((big_o[1:B + 1], big_l[1:B + 1]), base)
    for edge in (0, B + 1):
        assert bool((bits(big_o[edge]) == O_FILL).all()) and bool((fbits(big_l[edge]) == L_FILL).all())
    # several splits: two calls, and lse = None leaves o's bits
    q, lens, pl = ml.split_case(1, 16)
    base = decode(q, pl, lens)
    assert same(decode(q, pl, lens), base)
    o = torch.full((len(lens), 1, 16, DC), O_FILL, dtype=torch.int16, device=dev_).view(BF)
    c.fa2_decode_paged_mla_bf16(q.to(dev_), pl[0].to(dev_), pl[1].to(dev_), torch.tensor(lens, dtype=torch.int32, device=dev_), SCALE, o)
    torch.cuda.synchronize()
    assert torch.equal(bits(o.cpu()), bits(base[0]))


# ---------------------------------------------------------------------------------------------------- 7. append

APPEND_T, APPEND_CTX, APPEND_PAGE, APPEND_NMAX, APPEND_HQ = [43, 0, 1, 26, 5], [0, 7, 200, 64, 3], 16, 256, 5
MODES = ("none", "half", "interleaved")


def _append_problem():
    g = torch.Generator().manual_seed(43)
    lens = [c + t for c, t in zip(APPEND_CTX, APPEND_T)]
    pool, bt = ml.make_pool((torch.randn(len(lens), APPEND_NMAX, DK, generator=g)).to(BF), APPEND_PAGE, lens, seed=2)
    front, back = 3, 5
    cu = [front]
    for t in APPEND_T:
        cu.append(cu[-1] + t)
    total = cu[-1] + back
    c_new, k_pe, q = (torch.randn(total, *s, generator=g).to(BF) for s in ((DC,), (DR,), (APPEND_HQ, DK)))
    return lens, pool, bt, cu, c_new, k_pe, q


def run_append(c_new, k_pe, pool, bt, lens, cu, q, table, rope, in_place=False, dev="cuda"):
    cd, kd, pd, bd = (t.to(dev) for t in (c_new, k_pe, pool, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cud = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    qd = qo = None
    if q is not None:
        qd = q.to(dev)
        qo = qd if in_place else torch.full(qd.shape, Q_FILL, dtype=torch.int16, device=dev).view(BF)
    pkg().kv_append_paged_mla_bf16(cd, kd, pd, bd, sl, cud, qd, qo, None if table is None else table.to(dev), rope)
    torch.cuda.synchronize()
    assert torch.equal(bits(cd.cpu()), bits(c_new)) and torch.equal(bits(kd.cpu()), bits(k_pe))
    if q is not None and not in_place:
        assert torch.equal(bits(qd.cpu()), bits(q))
    return pd.cpu(), (qo.cpu() if qo is not None else None)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=MODES)
def test_append(built, dev, mode):
    """T_b = 43, 0, 1, 26, 5 behind 0, 7, 200, 64, 3 keys at page 16: runs that cross page edges, a sequence without a token. The 512 latent
    dims of the pool row and of q bit for bit; the 64 rotary dims within kv_append_bf16_reference's bound of the reference called on them as
    an Hkv = 1, D = 64 problem (rope none: bit for bit); every other pool row and the packed rows of no sequence untouched; q_out = q in place."""
    lens, pool, bt, cu, c_new, k_pe, q = _append_problem()
    table = None if mode == 0 else pkg().kv_append_rope_table(APPEND_NMAX, DR)
    got, qo = run_append(c_new, k_pe, pool, bt, lens, cu, q, table, MODES[mode])
    rot = pool[:, None, :, DC:].contiguous()
    kp, _, k_live, rows, dead = ar.ref_append_varlen(k_pe[:, None].contiguous(), k_pe[:, None].contiguous(), rot, rot, bt, lens, cu,
                                                     q[..., DC:].contiguous(), table, mode)
    assert len(rows) == sum(APPEND_T) and not dead and int(k_live.sum()) == sum(APPEND_T)
    assert torch.equal(bits(got[~k_live]), bits(pool[~k_live]))  # every row the call does not own, the 2^100 pages included
    assert any(pos % APPEND_PAGE == APPEND_PAGE - 1 for (_, _, pos, *_) in rows) and any(pos % APPEND_PAGE == 0 for (_, _, pos, *_) in rows)
    worst = 0.0
    for row, b, pos, k_rot, k_mag, q_rot, q_mag in rows:
        dst = got[int(bt[b, pos // APPEND_PAGE]), pos % APPEND_PAGE]
        assert torch.equal(bits(dst[:DC]), bits(c_new[row])), (row, "c")
        assert torch.equal(bits(qo[row, :, :DC]), bits(q[row, :, :DC])), (row, "q_nope")
        if mode == 0:
            assert torch.equal(bits(dst[DC:]), bits(k_pe[row])) and torch.equal(bits(qo[row, :, DC:]), bits(q[row, :, DC:])), row
            continue
        for what, have, want, mag in (("k_pe", dst[DC:].double(), k_rot[0], k_mag[0]), ("q_pe", qo[row, :, DC:].double(), q_rot, q_mag)):
            err, bnd = (have - want).abs(), ar.bound(want, mag)
            worst = max(worst, float((err / bnd.clamp(min=1e-300)).max()))
            assert bool((err <= bnd).all()), (row, what, float((err - bnd).max()))
    print("mla append rope=%s: rotary dims within %.4f of the bound" % (MODES[mode], worst))
    if mode != 0:  # the rotation did something: only a token at position 0 keeps its bits
        moved = sum(not torch.equal(bits(got[int(bt[b, pos // APPEND_PAGE]), pos % APPEND_PAGE, DC:]), bits(k_pe[row])) for row, b, pos, *_ in rows)
        assert moved >= len(rows) - 1, moved
    for sl in (slice(0, cu[0]), slice(cu[-1], None)):  # the packed rows of no sequence
        assert bool((bits(qo[sl]) == Q_FILL).all())
    got2, qi = run_append(c_new, k_pe, pool, bt, lens, cu, q, table, MODES[mode], in_place=True)
    seq = slice(cu[0], cu[-1])
    assert torch.equal(bits(got2), bits(got)) and torch.equal(bits(qi[seq]), bits(qo[seq]))
    assert torch.equal(bits(qi[:cu[0]]), bits(q[:cu[0]])) and torch.equal(bits(qi[cu[-1]:]), bits(q[cu[-1]:]))
    got3, none = run_append(c_new, k_pe, pool, bt, lens, cu, None, table, MODES[mode])  # without q: the pool's bits
    assert none is None and torch.equal(bits(got3), bits(got))


# ---------------------------------------------------------------------------------------------------- 8. chain

def test_chain_append_then_decode_eager_and_captured(built, dev):
    """The (2, 40) problem of the several-splits case: the two newest tokens of every sequence are appended (rope half), then all are attended
    to with the rotated q. Eager against the reference on the pool the append filled; then the same two calls captured in a graph and replayed on
    fresh buffers: bit for bit the eager result."""
    c = pkg()
    T, Hq = 2, 40
    q4, lens, (pool, bt) = ml.split_case(T, Hq)
    B = len(lens)
    g = torch.Generator().manual_seed(5)
    cu = list(range(0, T * B + 1, T))
    c_new, k_pe = ((torch.randn(T * B, d, generator=g) * SCALE).to(BF) for d in (DC, DR))
    q = q4.reshape(T * B, Hq, DK).contiguous()
    table = c.kv_append_rope_table(bt.shape[1] * pool.shape[1], DR)
    S, _, need = plan(B, T, Hq, (pool, bt))
    assert S > 1
    dv = "cuda"
    fixed = tuple(t.to(dv) for t in (c_new, k_pe, bt, torch.tensor(lens, dtype=torch.int32), torch.tensor(cu, dtype=torch.int32), q, table))

    def buffers():
        return (pool.to(dv), torch.full(q.shape, Q_FILL, dtype=torch.int16, device=dv).view(BF),
                torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=dv).view(BF),
                torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=dv).view(torch.float32), torch.empty(need, dtype=torch.uint8, device=dv))

    def step(pl, qo, o, lse, ws):
        cn, kp_, btd, sl, cud, qd, tb = fixed
        c.kv_append_paged_mla_bf16(cn, kp_, pl, btd, sl, cud, qd, qo, tb, "half")
        c.fa2_decode_paged_mla_bf16(qo.view(B, T, Hq, DK), pl, btd, sl, SCALE, o, lse, ws)

    eager = buffers()
    step(*eager)
    torch.cuda.synchronize()
    pl, qo, o, lse = (t.cpu() for t in eager[:4])
    assert bool((qo[cu[4]:] == 0).all())  # the sequence of length 0: its two tokens stand below position 0, q_out rows are zero
    ref = ml.decode(qo.view(B, T, Hq, DK), pl, bt, lens, SCALE)
    note("chain", check(o, lse, *ref, "mla chain append + decode T=%d Hq=%d S=%d" % (T, Hq, S)))
    assert not torch.equal(bits(pl), bits(pool))
    graph_bufs = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(*graph_bufs)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("pool", "q_out", "o"), graph_bufs[:3], (pl, qo, o)):
        assert torch.equal(bits(a.cpu()), bits(b)), name
    assert torch.equal(fbits(graph_bufs[3].cpu()), fbits(lse))


def test_zz_summary_of_error_over_bound(built, dev):
    """The RATIOS table: the largest O err / bound of every group of parity cases of this file. Not an assertion of its own --
    every case asserted err <= bound where it ran."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
