"""GPU: multi-head latent attention over a paged latent cache held in FP8 -- cuda_learn_notes_amd.fa2_decode_paged_mla_bf16_fp8,
kv_append_paged_mla_bf16_fp8 and kv_gather_paged_mla_bf16_fp8 (csrc/*_mla_bf16_fp8.*) -- against
tests/paged_mla_fp8_reference.py (fp64 on the dequantised pool and the bf16 emulation on the codes, anchored to the bf16 MLA reference by
tests/test_paged_mla_fp8_surface.py) and tests/fp8_kv_reference.py (quantize byte for byte, bound for the rotated dims). No new tolerance: O
within paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol per head, -inf LSE entries and zero rows exactly
(test_gpu_paged_sink_attention.check). Beyond parity: bit equality with the bf16 entry on the dequantised pool at a power-of-two scale, every
finite code, exact counts, the rotary dims, dead pages, guard bands, the append, the gather, and a chain with a captured graph. Every parity
case prints err / bound before it asserts (pytest -s); the last test prints the largest per group.

Largest err / bound of O seen on an MI355X: see DESIGN 4.4.19 and profiles/r29_paged_mla_fp8_tests.log."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import kv_append_bf16_reference as ar  # noqa: E402
import paged_edge_cases as ec  # noqa: E402
import paged_mla_fp8_reference as mf  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F8 = torch.bfloat16, f8.F8
DC, DR, DK, SCALE = ml.DC, ml.DR, ml.DK, ml.SCALE
O_FILL, L_FILL, Q_FILL, MARK = sk.O_FILL, sk.L_FILL, 0x3C5A, 0x5B
NEG_INF = float("-inf")
P2 = 2.0 ** -8
bits, fbits, check, cbits = sk.bits, sk.fbits, sk.check, f8.bits
RATIOS = {}
DEV = "cuda"


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def plan(B, T, Hq, pool):
    return pkg().fa2_decode_paged_mla_bf16_fp8_plan(B, T, Hq, pool[1].shape[1], pool[0].shape[1])


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def decode(q, pool, lens, kvs, scale=SCALE, bf16=False):
    """(o, lse) on the CPU; the workspace is sized from the entry's own plan. bf16: the bf16 MLA entry on a bf16 pool instead."""
    c = pkg()
    qd, pd, bd = (t.to(DEV) for t in (q, *pool))
    B, T, Hq, _ = q.shape
    o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=DEV).view(BF)
    lse = torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=DEV).view(torch.float32)
    ws = torch.empty(max(plan(B, T, Hq, pool)[2], 16), dtype=torch.uint8, device=DEV)
    if bf16:
        c.fa2_decode_paged_mla_bf16(qd, pd, bd, i32(lens), scale, o, lse, ws)
    else:
        c.fa2_decode_paged_mla_bf16_fp8(qd, pd, bd, i32(lens), mf.scale_t(kvs).to(DEV), scale, o, lse, ws)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def same(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(fbits(a[1]), fbits(b[1]))


def deq_bf16(pool, bt, lens, kvs):
    """The pool dequantised to bf16 (exact at a power-of-two scale), the dead pages zero."""
    x = mf.dequantize(mf.zero_dead_pages(pool, bt, lens), kvs, torch.float64)
    assert torch.equal(x.to(BF).double(), x)
    return x.to(BF)


# ---------------------------------------------------------------------------------------------------- 1. one split

@pytest.mark.parametrize("kvs", mf.KV_SCALES, ids=["kv2^-8", "kv0.003"])
@pytest.mark.parametrize("page", mf.ONE_PAGES)
@pytest.mark.parametrize("TH", mf.ONE_TH, ids=lambda th: "T%dxHq%d" % th)
def test_decode_one_split(built, dev, TH, page, kvs):
    """paged_mla_reference's lengths (0, 1, 17, 63, 64, 65, 100, 257; at T = 8 lengths below T) and rows from 1 to four row groups, quantised on
    the CPU."""
    T, Hq = TH
    q, lens, pool = mf.one_case(T, Hq, page, kvs)
    assert plan(len(lens), T, Hq, pool)[0] == 1
    got = decode(q, pool, lens, kvs)
    ro, rl, emul = mf.decode(q, *pool, lens, kvs, SCALE)
    assert bool((rl[0] == NEG_INF).all())
    note("decode, one split", check(*got, ro, rl, emul, "mla fp8 S=1 T=%d Hq=%d page=%d kv_scale=%g" % (T, Hq, page, kvs)))


# ---------------------------------------------------------------------------------------------------- 2. several splits

@pytest.mark.parametrize("kvs", mf.KV_SCALES, ids=["kv2^-8", "kv0.003"])
@pytest.mark.parametrize("TH", mf.SPLIT_TH, ids=lambda th: "T%dxHq%d" % th)
def test_decode_several_splits(built, dev, TH, kvs):
    """B = 5 at page 16 with 64 table entries: 4 splits of 256 keys; the sequence of length 0 is still written by the combine."""
    T, Hq = TH
    q, lens, pool = mf.split_case(T, Hq, kvs)
    S, C, _ = plan(len(lens), T, Hq, pool)
    assert (S, C) == (4, 256), (S, C)
    got = decode(q, pool, lens, kvs)
    ro, rl, emul = mf.decode(q, *pool, lens, kvs, SCALE)
    note("decode, several splits", check(*got, ro, rl, emul, "mla fp8 S=%d T=%d Hq=%d kv_scale=%g" % (S, T, Hq, kvs)))
    assert bool((bits(got[0][4]) == 0).all()) and bool((got[1][4] == NEG_INF).all())


# ---------------------------------------------------------------------------------------------------- 2b. a scale that is not the data's

@pytest.mark.parametrize("kvs", mf.KV_SCALES, ids=["kv2^-8", "kv0.003"])
@pytest.mark.parametrize("scale", ml.OTHER_SCALES, ids=["yarn", "quarter"])
@pytest.mark.parametrize("case", ml.SCALE_TH, ids=lambda c: "T%dxHq%d%s" % (c[0], c[1], "-split" if c[2] else ""))
def test_decode_at_a_scale_that_is_not_the_datas(built, dev, case, scale, kvs):
    """The one-split case at (3, 5) and the several-splits case at (2, 40) at V3's YaRN scale and at SCALE / 4, at both pool scales, q x Q_MULT:
    the reference at SCALE is more than 20 x o_bound away (proven without a GPU by tests/test_paged_mla_fp8_surface.py), so a constant in the
    scale_log2 kv_scale product would show."""
    T, Hq, split = case
    q, lens, pool, ref, ref0 = mf.scale_case(T, Hq, split, kvs, scale)
    S = plan(len(lens), T, Hq, pool)[0]
    assert (S > 1) == split
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla fp8 scale %.5f kv_scale %g T=%d Hq=%d S=%d: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, kvs, T, Hq, S, diff, need))
    assert diff > need
    note("decode, another scale", check(*decode(q, pool, lens, kvs, scale=scale), *ref, "mla fp8 scale=%.5f kv_scale=%g S=%d T=%d Hq=%d" % (scale, kvs, S, T, Hq)))


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
    """The several-splits case at (2, 40) at YARN, kv_scale 0.003: the stream kernel and the combine captured and replayed, bit for bit the
    eager result."""
    c = pkg()
    T, Hq, kvs = 2, 40, mf.KV_SCALES[1]
    q, lens, pool, ref, _ = mf.scale_case(T, Hq, True, kvs, ml.YARN)
    B = len(lens)
    S, _, need = plan(B, T, Hq, pool)
    assert S > 1
    fixed = (q.to(DEV), pool[0].to(DEV), pool[1].to(DEV), i32(lens), mf.scale_t(kvs).to(DEV))
    o, lse = _graph_replays_eager(lambda o, lse, ws: c.fa2_decode_paged_mla_bf16_fp8(*fixed, ml.YARN, o, lse, ws), B, T, Hq, need)
    note("decode, another scale", check(o, lse, *ref, "mla fp8 scale=YARN eager, then a captured graph S=%d" % S))


# ---------------------------------------------------------------------------------------------------- 3. bit equality with the bf16 entry

def _bit_cases(T, Hq):
    """One split at pages 16 and 64, and several splits: split_case's pool and lengths; at (2, 128), which split_case does not have, with the
    queries of (1, 128) and their mirror over the heads as the two tokens."""
    yield mf.one_case(T, Hq, 16, P2)
    yield mf.one_case(T, Hq, 64, P2)
    if (T, Hq) in mf.SPLIT_TH:
        yield mf.split_case(T, Hq, P2)
    else:
        q, lens, pool = mf.split_case(1, Hq, P2)
        yield torch.cat([q, q.flip(2)], dim=1).contiguous(), lens, pool


@pytest.mark.parametrize("TH", [(1, 16), (2, 128)], ids=lambda th: "T%dxHq%d" % th)
def test_bits_of_the_bf16_entry_at_a_power_of_two_scale(built, dev, TH):
    """kv_scale = 2^-8: the pool dequantised to bf16 is exact, every product with the scale is exact, and the body behind the staging is the
    sibling's: O and LSE are fa2_decode_paged_mla_bf16's on the dequantised pool, bit for bit, with one split and with several."""
    T, Hq = TH
    splits = []
    for q, lens, (pool, bt) in _bit_cases(T, Hq):
        assert q.shape[1:3] == (T, Hq)
        S = plan(len(lens), T, Hq, (pool, bt))[0]
        splits.append(S)
        a = decode(q, (pool, bt), lens, P2)
        b = decode(q, (deq_bf16(pool, bt, lens, P2), bt), lens, P2, bf16=True)
        assert same(a, b), (T, Hq, S)
        assert bool((a[1][0] == NEG_INF).all() if lens[0] == 0 else torch.isfinite(a[1][0]).all())
    assert splits[:2] == [1, 1] and splits[2] > 1, splits


# ---------------------------------------------------------------------------------------------------- 4. every finite code

@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("kvs", [1.0, P2], ids=["kv1", "kv2^-8"])
def test_every_finite_code(built, dev, kvs, n):
    """q = 0 over n identical rows whose 512 value dims hold all 254 finite codes (subnormals and -0 included, repeated to 512): every weight is
    1 / n, a power of two, so O is e4m3(code) kv_scale bit for bit. The one exception is the sign of the code -0: the fp32 accumulator starts at +0
    and +0 + -0 is +0 in IEEE arithmetic (in the bf16 entry as well), so that dim is compared as a value (0 == -0) and its bits are printed."""
    codes = mf.all_finite_codes()
    raw = torch.cat([codes, codes, codes[:4], torch.zeros(DR, dtype=torch.uint8)])
    assert raw.numel() == DK and len(set(raw[:DC].tolist())) == 254
    row = raw.view(F8)
    pool = mf.make_pool(raw[None, None].expand(1, 16, DK).contiguous().view(F8), 16, [n], seed=4)
    q = torch.zeros(1, 1, 16, DK, dtype=BF)
    o, lse = decode(q, pool, [n], kvs)
    want = (row[:DC].double() * kvs).to(BF)
    assert torch.equal(want.double(), row[:DC].double() * kvs)
    want = want.expand(1, 1, 16, DC)
    nz = want != 0
    print("every code n=%d kv_scale=%g: the bits of O over the code -0: %s" % (n, kvs, sorted(set(bits(o)[~nz].tolist()))))
    assert torch.equal(o.double(), want.double())               # every code exactly, the two zeros as zero
    assert torch.equal(bits(o)[nz], bits(want)[nz]), n          # and bit for bit; an accumulator that starts at +0 gives +0 + -0 = +0
    assert float((lse.double() - math.log(n)).abs().max()) <= ec.lse_tol_at(n)


# ---------------------------------------------------------------------------------------------------- 5. exact counts

@pytest.mark.parametrize("max_pages", [20, 64], ids=["one-split", "several-splits"])
@pytest.mark.parametrize("TH", [(1, 16), (3, 5)], ids=lambda th: "T%dxHq%d" % th)
def test_exact_counts(built, dev, TH, max_pages):
    """q = 0, value codes = 1.0, rotary codes random: every weight of a row is 1 / n, so O is exactly kv_scale and LSE = ln n."""
    T, Hq = TH
    lens, page, kvs = ml.COUNT_N, 16, P2
    g = torch.Generator().manual_seed(max_pages)
    dense = torch.ones(1, max_pages * page, DK)
    dense[..., DC:] = torch.randn(1, max_pages * page, DR, generator=g)
    pool = mf.make_pool(dense.to(F8).expand(len(lens), -1, -1).contiguous(), page, lens, seed=3)
    S = plan(len(lens), T, Hq, pool)[0]
    assert (S == 1) == (max_pages == 20), S
    q = torch.zeros(len(lens), T, Hq, DK, dtype=BF)
    o, lse = decode(q, pool, lens, kvs)
    worst = 0.0
    for b, n_b in enumerate(lens):
        for t in range(T):
            n = max(n_b - (T - 1 - t), 0)
            if n == 0:
                assert bool((bits(o[b, t]) == 0).all()) and bool((lse[b, t] == NEG_INF).all()), (b, t)
                continue
            assert bool((o[b, t] == kvs).all()), (b, t, n)
            err, tol = (lse[b, t].double() - math.log(n)).abs().max().item(), ec.lse_tol_at(n)
            worst = max(worst, err / tol)
            assert err <= tol, (b, t, n, err, tol)
    print("mla fp8 counts T=%d Hq=%d S=%d: LSE = ln(visible keys) within %.4f of the tolerance" % (T, Hq, S, worst))


# ---------------------------------------------------------------------------------------------------- 6. the rotary dims

def test_rotary_dims_count_in_the_score_and_not_in_the_value(built, dev):
    """Other codes in bytes 512 ... 575 of the visible rows change LSE; with q's rotary dims zero they change nothing, bit for bit."""
    for (T, Hq), case in (((3, 5), mf.one_case(3, 5, 16, 0.003)), ((2, 40), mf.split_case(2, 40, 0.003))):
        q, lens, (pool, bt) = case
        other = cbits(pool).clone()
        other[..., DC:] ^= 0x80  # the sign of every rotary code: a finite code stays finite, a dead page's NaN bytes stay NaN
        other = other.view(F8)
        a, b = decode(q, (pool, bt), lens, 0.003), decode(q, (other, bt), lens, 0.003)
        fin = torch.isfinite(a[1])
        assert not torch.equal(fbits(a[1][fin]), fbits(b[1][fin])) and float((a[1][fin] - b[1][fin]).abs().max()) > 1e-4
        note("decode, other rotary codes", check(*b, *mf.decode(q, other, bt, lens, 0.003, SCALE), "mla fp8 other k_pe T=%d Hq=%d" % (T, Hq)))
        q0 = q.clone()
        q0[..., DC:] = 0
        assert same(decode(q0, (pool, bt), lens, 0.003), decode(q0, (other, bt), lens, 0.003)), (T, Hq)


# ---------------------------------------------------------------------------------------------------- 7. dead pages

def test_dead_pages_and_table_entries_are_never_followed(built, dev):
    """The pages no live entry names hold the NaN byte, and the table entries past ceil(len / page) point at one: the result has the bits of a
    pool whose dead pages hold zeros, and of a table whose dead entries are 0."""
    for case, kvs in ((mf.one_case(1, 17, 16, 0.003), 0.003), (mf.one_case(8, 3, 64, P2), P2), (mf.split_case(1, 16, 0.003), 0.003)):
        q, lens, (pool, bt) = case
        assert bool((cbits(pool[-1]) == f8.NAN_BYTE).all())
        base = decode(q, (pool, bt), lens, kvs)
        assert bool(torch.isfinite(base[0].float()).all())
        assert same(base, decode(q, (mf.zero_dead_pages(pool, bt, lens), bt), lens, kvs))
        bt0 = bt.clone()
        for b, n in enumerate(lens):
            bt0[b, -(-n // pool.shape[1]):] = 0
        assert not torch.equal(bt0, bt) and same(base, decode(q, (pool, bt0), lens, kvs))


# ---------------------------------------------------------------------------------------------------- 8. guard bands, two calls

def test_guard_bands_and_two_calls(built, dev):
    c = pkg()
    for q, lens, (pool, bt), kvs in ((*mf.one_case(1, 16, 16, 0.003), 0.003), (*mf.split_case(1, 16, 0.003), 0.003)):
        B, T, Hq, _ = q.shape
        base = decode(q, (pool, bt), lens, kvs)
        assert same(decode(q, (pool, bt), lens, kvs), base)  # two calls
        need = plan(B, T, Hq, (pool, bt))[2]
        big_o = torch.full((B + 2, T, Hq, DC), O_FILL, dtype=torch.int16, device=DEV).view(BF)
        big_l = torch.full((B + 2, T, Hq), L_FILL, dtype=torch.int32, device=DEV).view(torch.float32)
        big_w = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=DEV)
        ws = big_w[256:256 + need] if need else None
        c.fa2_decode_paged_mla_bf16_fp8(q.to(DEV), pool.to(DEV), bt.to(DEV), i32(lens), mf.scale_t(kvs).to(DEV), SCALE, big_o[1:B + 1], big_l[1:B + 1], ws)
        torch.cuda.synchronize()
        big_o, big_l, big_w = big_o.cpu(), big_l.cpu(), big_w.cpu()
        assert same((big_o[1:B + 1], big_l[1:B + 1]), base)
        for edge in (0, B + 1):
            assert bool((bits(big_o[edge]) == O_FILL).all()) and bool((fbits(big_l[edge]) == L_FILL).all())
        assert bool((big_w[:256] == 0xA5).all()) and bool((big_w[256 + need:] == 0xA5).all())
        o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=DEV).view(BF)  # lse = None leaves o's bits
        c.fa2_decode_paged_mla_bf16_fp8(q.to(DEV), pool.to(DEV), bt.to(DEV), i32(lens), mf.scale_t(kvs).to(DEV), SCALE, o)
        torch.cuda.synchronize()
        assert torch.equal(bits(o.cpu()), bits(base[0]))


# ---------------------------------------------------------------------------------------------------- 9. append

APPEND_T, APPEND_CTX, APPEND_PAGE, APPEND_NMAX, APPEND_HQ = [43, 0, 1, 26, 5], [0, 7, 200, 64, 3], 16, 256, 5
MODES = ("none", "half", "interleaved")


def _append_problem():
    g = torch.Generator().manual_seed(43)
    lens = [c + t for c, t in zip(APPEND_CTX, APPEND_T)]
    dense = torch.full((len(lens), APPEND_NMAX, DK), MARK, dtype=torch.uint8).view(F8)
    pool, bt = mf.make_pool(dense, APPEND_PAGE, lens, seed=2)
    pool = torch.full(pool.shape, MARK, dtype=torch.uint8).view(F8)  # every byte the marker, the dead pages too
    front, back = 3, 5
    cu = [front]
    for t in APPEND_T:
        cu.append(cu[-1] + t)
    total = cu[-1] + back
    c_new, k_pe, q = ((torch.randn(total, *s, generator=g) * SCALE).to(BF) for s in ((DC,), (DR,), (APPEND_HQ, DK)))
    return lens, pool, bt, cu, c_new, k_pe, q


def run_append(c_new, k_pe, pool, bt, lens, cu, q, table, rope, kvs, bf16_pool=None):
    cd, kd, bd = (t.to(DEV) for t in (c_new, k_pe, bt))
    pd = (pool if bf16_pool is None else bf16_pool).to(DEV)
    qd = qo = None
    if q is not None:
        qd = q.to(DEV)
        qo = torch.full(qd.shape, Q_FILL, dtype=torch.int16, device=DEV).view(BF)
    tb = None if table is None else table.to(DEV)
    if bf16_pool is None:
        pkg().kv_append_paged_mla_bf16_fp8(cd, kd, pd, bd, i32(lens), i32(cu), mf.scale_t(kvs).to(DEV), qd, qo, tb, rope)
    else:
        pkg().kv_append_paged_mla_bf16(cd, kd, pd, bd, i32(lens), i32(cu), qd, qo, tb, rope)
    torch.cuda.synchronize()
    assert torch.equal(bits(cd.cpu()), bits(c_new)) and torch.equal(bits(kd.cpu()), bits(k_pe))
    return pd.cpu(), (qo.cpu() if qo is not None else None)


@pytest.mark.parametrize("kvs", mf.KV_SCALES, ids=["kv2^-8", "kv0.003"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=MODES)
def test_append(built, dev, mode, kvs):
    """T_b = 43, 0, 1, 26, 5 behind 0, 7, 200, 64, 3 keys at page 16 into a pool of marker bytes: c, and k_pe under rope none, byte for byte
    fp8_kv_reference.quantize; rotated k_pe within fp8_kv_reference.bound of the fp64 rotation (kv_append_bf16_reference on the rotary dims as
    an Hkv = 1, D = 64 problem); q_out the bits of the bf16 MLA append; every other byte still the marker."""
    lens, pool, bt, cu, c_new, k_pe, q = _append_problem()
    table = None if mode == 0 else pkg().kv_append_rope_table(APPEND_NMAX, DR)
    got, qo = run_append(c_new, k_pe, pool, bt, lens, cu, q, table, MODES[mode], kvs)
    _, qo_bf = run_append(c_new, k_pe, pool, bt, lens, cu, q, table, MODES[mode], kvs, bf16_pool=torch.zeros(pool.shape, dtype=BF))
    assert torch.equal(bits(qo), bits(qo_bf))
    rot = torch.zeros(pool.shape[0], 1, APPEND_PAGE, DR, dtype=BF)
    _, _, k_live, rows, dead = ar.ref_append_varlen(k_pe[:, None].contiguous(), k_pe[:, None].contiguous(), rot, rot, bt, lens, cu,
                                                    q[..., DC:].contiguous(), table, mode)
    assert len(rows) == sum(APPEND_T) and not dead and int(k_live.sum()) == sum(APPEND_T)
    gb = cbits(got)
    assert bool((gb[~k_live] == MARK).all()) and not bool((gb[k_live][:, :DC] == MARK).all(dim=1).any())  # every row the call does not own
    s64 = torch.tensor(mf.scale_t(kvs).item(), dtype=torch.float64)
    worst = 0.0
    for row, b, pos, k_rot, k_mag, q_rot, q_mag in rows:
        dst = got[int(bt[b, pos // APPEND_PAGE]), pos % APPEND_PAGE]
        assert torch.equal(cbits(dst[:DC]), cbits(mf.quantize(c_new[row], kvs))), (row, "c")
        if mode == 0:
            assert torch.equal(cbits(dst[DC:]), cbits(mf.quantize(k_pe[row], kvs))), (row, "k_pe")
            continue
        err = (dst[DC:].double() * s64 - k_rot[0]).abs()
        bnd = f8.bound(k_rot[0], float(s64), k_mag[0])
        worst = max(worst, float((err / bnd).max()))
        assert bool((err <= bnd).all()), (row, float((err / bnd).max()))
    print("mla fp8 append rope=%s kv_scale=%g: rotated k_pe within %.4f of the bound" % (MODES[mode], kvs, worst))
    got2, none = run_append(c_new, k_pe, pool, bt, lens, cu, None, table, MODES[mode], kvs)  # without q: the pool's bytes
    assert none is None and torch.equal(cbits(got2), gb)


# ---------------------------------------------------------------------------------------------------- 10. gather

def run_gather(pool, bt, cu, kvs, total, starts=None, fill=Q_FILL):
    out = torch.full((total, DK), fill, dtype=torch.int16, device=DEV).view(BF)
    pkg().kv_gather_paged_mla_bf16_fp8(pool.to(DEV), bt.to(DEV), i32(cu), mf.scale_t(kvs).to(DEV), out, None if starts is None else i32(starts))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("kvs", mf.KV_SCALES, ids=["kv2^-8", "kv0.003"])
def test_gather(built, dev, kvs):
    """Packed row cu_k[b] + i = cache row starts[b] + i as dequantize(codes, kv_scale, float32).bfloat16(), bit for bit, with and without starts;
    rows past the table are zeros; packed rows of no sequence keep their fill."""
    q, lens, (pool, bt) = mf.split_case(1, 16, kvs)
    Nmax = bt.shape[1] * pool.shape[1]
    dense = ml.gather(mf.dequantize(mf.zero_dead_pages(pool, bt, lens), kvs, torch.float32).to(BF), bt, lens)
    for starts, counts in ((None, [n for n in lens]), ([990, 17, 250, 0, 0], [50, 100, 7, 100, 0])):
        cu = [2]
        for n in counts:
            cu.append(cu[-1] + n)
        total = cu[-1] + 3
        out = run_gather(pool, bt, cu, kvs, total, starts)
        assert bool((bits(out[:2]) == Q_FILL).all()) and bool((bits(out[cu[-1]:]) == Q_FILL).all())
        for b, n in enumerate(counts):
            s0 = 0 if starts is None else starts[b]
            live = max(min(n, lens[b] - s0), 0)  # the rows the sequence owns; behind them only the rows at or past the table are defined
            assert torch.equal(bits(out[cu[b]:cu[b] + live]), bits(dense[b, s0:s0 + live])), b
            past = max(Nmax - s0, 0)
            if n > past:
                assert bool((bits(out[cu[b] + past:cu[b] + n]) == 0).all()), b
    assert starts[0] + counts[0] > Nmax  # the first sequence of the second round runs past the table


def test_gather_returns_what_the_append_wrote(built, dev):
    kvs = 0.003
    lens, pool, bt, cu, c_new, k_pe, q = _append_problem()
    got, _ = run_append(c_new, k_pe, pool, bt, lens, cu, None, None, "none", kvs)
    cuk = [0]
    for t in APPEND_T:
        cuk.append(cuk[-1] + t)
    out = run_gather(got, bt, cuk, kvs, cuk[-1], starts=APPEND_CTX)
    new = torch.cat([c_new, k_pe], dim=-1)[cu[0]:cu[-1]]
    want = mf.dequantize(mf.quantize(new, kvs), kvs, torch.float32).to(BF)
    assert torch.equal(bits(out), bits(want))


# ---------------------------------------------------------------------------------------------------- 11. chain and graph

def test_chain_append_then_decode_eager_and_captured(built, dev):
    """[130, 7] tokens appended with the interleaved rotation into an empty FP8 pool, one more token per sequence, one decode step at Hq 16
    against the reference that quantises on the CPU; then append -> decode captured once on one stream and replayed with lengths, rows and table
    changed in place: bit-equal to the eager calls."""
    c = pkg()
    kvs, Hq, page, max_pages, B = 0.003, 16, 16, 16, 2
    g = torch.Generator().manual_seed(9)
    prompt, P = [130, 7], 40
    table = c.kv_append_rope_table(max_pages * page, DR)
    perm = torch.randperm(P, generator=g).to(torch.int32)
    bt = perm[:B * max_pages].reshape(B, max_pages).contiguous()  # distinct pages; perm[32:] are named by no entry
    rnd = lambda *s: (torch.randn(*s, generator=g) * SCALE).to(BF)  # noqa: E731
    c0, k0 = rnd(sum(prompt), DC), rnd(sum(prompt), DR)
    c1, k1, q1 = rnd(B, DC), rnd(B, DR), rnd(B, Hq, DK)
    c2, k2, q2 = rnd(B, DC), rnd(B, DR), rnd(B, Hq, DK)
    cx, kx = rnd(8, DC), rnd(8, DR)  # 8 more tokens of sequence 1 between the steps: its next token then opens page 1
    bt2 = bt.clone()
    bt2[1, 1] = perm[B * max_pages]  # not yet written in step 1: the entry changes in place, and step 2 writes and reads the page it names
    sc = mf.scale_t(kvs).to(DEV)
    tb = table.to(DEV)

    def state():
        return dict(pool=torch.full((P, page, DK), f8.NAN_BYTE, dtype=torch.uint8, device=DEV).view(F8), bt=bt.to(DEV),
                    sl=i32(prompt), cu=i32([0, 1, 2]), cn=c1.to(DEV), kp=k1.to(DEV), q=q1.to(DEV),
                    qo=torch.full((B, Hq, DK), Q_FILL, dtype=torch.int16, device=DEV).view(BF),
                    o=torch.full((B, 1, Hq, DC), O_FILL, dtype=torch.int16, device=DEV).view(BF),
                    lse=torch.full((B, 1, Hq), L_FILL, dtype=torch.int32, device=DEV).view(torch.float32))

    def prefill(s):
        c.kv_append_paged_mla_bf16_fp8(c0.to(DEV), k0.to(DEV), s["pool"], s["bt"], s["sl"], i32([0, prompt[0], sum(prompt)]), sc, None, None, tb,
                                       "interleaved")

    def step(s):
        c.kv_append_paged_mla_bf16_fp8(s["cn"], s["kp"], s["pool"], s["bt"], s["sl"], s["cu"], sc, s["q"], s["qo"], tb, "interleaved")
        c.fa2_decode_paged_mla_bf16_fp8(s["qo"].view(B, 1, Hq, DK), s["pool"], s["bt"], s["sl"], sc, SCALE, s["o"], s["lse"])

    LENS = {1: [prompt[0] + 1, prompt[1] + 1], 2: [prompt[0] + 2, prompt[1] + 10]}

    def advance(s, k):  # the inputs of step k, in place
        if k == 2:  # outside the graph: sequence 1 grows by 8 rows (positions 8 ... 15), sequence 0 by none
            c.kv_append_paged_mla_bf16_fp8(cx.to(DEV), kx.to(DEV), s["pool"], s["bt"], i32([prompt[0] + 1, prompt[1] + 9]), i32([0, 0, 8]), sc, None,
                                           None, tb, "interleaved")
        s["sl"].copy_(i32(LENS[k]))
        if k == 2:
            s["bt"].copy_(bt2.to(DEV))
            s["cn"].copy_(c2.to(DEV)), s["kp"].copy_(k2.to(DEV)), s["q"].copy_(q2.to(DEV))

    assert plan(B, 1, Hq, (torch.empty(P, page, DK), bt))[0] == 1
    e = state()
    prefill(e)
    results = []
    for k in (1, 2):
        advance(e, k)
        step(e)
        torch.cuda.synchronize()
        results.append(tuple(e[x].cpu() for x in ("pool", "qo", "o", "lse")))
    # the eager steps against the reference on the pool the appends filled
    for k, (pl, qo, o, lse) in zip((1, 2), results):
        lens = LENS[k]
        tab = bt if k == 1 else bt2
        ref = mf.decode(qo.view(B, 1, Hq, DK), pl, tab, lens, kvs, SCALE)
        note("chain", check(o, lse, *ref, "mla fp8 chain step %d" % k))
    # the newest row of sequence 1 after step 1 is quantize() of the rotated input: c byte for byte
    pl = results[0][0]
    pos = prompt[1]
    assert torch.equal(cbits(pl[int(bt[1, pos // page]), pos % page, :DC]), cbits(mf.quantize(c1[1], kvs)))
    assert LENS[2][1] - 1 == page and int(bt2[1, 1]) != int(bt[1, 1])  # the newest token of sequence 1 in step 2 is row 0 of the changed entry
    assert not torch.equal(results[1][0][int(bt2[1, 1])].view(torch.uint8), results[0][0][int(bt2[1, 1])].view(torch.uint8))
    gs = state()
    prefill(gs)
    advance(gs, 1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(gs)
    torch.cuda.synchronize()
    for k in (1, 2):
        advance(gs, k)
        graph.replay()
        torch.cuda.synchronize()
        for name, want in zip(("pool", "qo", "o"), results[k - 1][:3]):
            have = gs[name].cpu()
            assert torch.equal(have.view(torch.uint8) if name == "pool" else bits(have), want.view(torch.uint8) if name == "pool" else bits(want)), (k, name)
        assert torch.equal(fbits(gs["lse"].cpu()), fbits(results[k - 1][3])), k


def test_zz_summary_of_error_over_bound(built, dev):
    """The RATIOS table: the largest O err / bound of every group of parity cases of this file. Not an assertion of its own --
    every case asserted err <= bound where it ran."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
