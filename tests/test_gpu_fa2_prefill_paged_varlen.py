"""GPU: packed variable-length prefill attention over a paged KV cache (cuda_learn_notes_amd.fa2_prefill_paged_varlen,
cln_fa2_prefill_paged_varlen; csrc/flash_attn_prefill_paged_varlen.cuh) against the per-sequence fp64 reference of
tests/prefill_varlen_reference.py and, bit for bit, against the fixed-T entry fa2_prefill_paged called on every sequence alone. Pools come from
paged_decode_reference.make_pool (NaN poison pages, shuffled placement); q / out carry 5 spare rows behind cu_q[B], and out / lse are pre-filled
with NaN, so a row the kernel must not touch keeps its NaN bits. Tolerances: decode_reference.fa_tol / lse_tol; -inf LSE entries and zero rows
are compared exactly. Every parity case prints its figures before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import prefill_varlen_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu

DS = [64, 128]
SPARE = 5
CASE_IDS = ["x".join(map(str, g)) for g, _ in vr.CASES]
bits = lambda t: t.view(torch.int16)  # noqa: E731
fbits = lambda t: t.view(torch.int32)  # noqa: E731


def contexts(geom, T):
    """Lengths len_b = context_b + T_b with the contexts {0, 1, page-1, page, 63, 64, 65, Nmax - T_b} dealt over the batch, shifted by `k`."""
    _, _, page, mp = geom
    Nmax = page * mp
    return lambda k: [min(c, Nmax - t) + t for c, t in
                      zip(([0, 1, page - 1, page, 63, 64, 65, Nmax] * 2)[k:k + len(T)], T)]


@functools.lru_cache(maxsize=None)
def problem(ci, D, seed=0):
    """Gaussian fp16 (q_b [T_b,Hq,D] per sequence, dense k, v [B,Hkv,Nmax,D]) on the CPU, made once per case and never modified."""
    (Hkv, G, page, mp), T = vr.CASES[ci]
    g = torch.Generator().manual_seed(1000 * seed + 97 * ci + D)
    qs = tuple(torch.randn(t, Hkv * G, D, generator=g).half() for t in T)
    k, v = (torch.randn(len(T), Hkv, page * mp, D, generator=g).half() for _ in range(2))
    return qs, k, v


def pack(qs, first=0, spare=SPARE):
    """(q [total_q,Hq,D], cu): the sequences packed from row `first` on, the rows in front and the `spare` rows behind filled with 6e4."""
    cu = vr.cu_of([x.shape[0] for x in qs], first)
    q = torch.full((cu[-1] + spare,) + tuple(qs[0].shape[1:]), 6e4, dtype=torch.half)
    for b, x in enumerate(qs):
        q[cu[b]:cu[b + 1]] = x
    return q, cu


def run(q, kp, vp, bt, lens, cu, want_lse=True, dev="cuda"):
    import cuda_learn_notes_amd as pkg
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    o = torch.full_like(qd, float("nan"))
    lse = torch.full(qd.shape[:2], float("nan"), dtype=torch.float32, device=dev) if want_lse else None
    pkg.fa2_prefill_paged_varlen(qd, kd, vd, bd, sl, cd, o, lse)
    torch.cuda.synchronize()
    return o.cpu(), (lse.cpu() if want_lse else None)


def untouched(o, lse, cu):
    """The rows outside [cu[0], cu[B]) keep their NaN fill, bit for bit."""
    nan16, nan32 = bits(torch.full((1,), float("nan"), dtype=torch.half)).item(), fbits(torch.full((1,), float("nan"))).item()
    for sl in (slice(0, cu[0]), slice(cu[-1], None)):
        assert bool((bits(o[sl]) == nan16).all()) and bool((fbits(lse[sl]) == nan32).all()), cu


def check(o, lse, q, kp, vp, bt, lens, cu, what):
    """The rows of the sequences: O within fa_tol(ref), LSE within lse_tol(ref), -inf LSE entries and their zero rows exactly."""
    ro, rl = vr.ref_prefill_paged_varlen(q, kp, vp, bt, lens, cu)
    untouched(o, lse, cu)
    o, lse, ro, rl = (t[cu[0]:cu[-1]] for t in (o, lse, ro, rl))
    assert bool(torch.isfinite(o).all()), what
    eo, bo = (o.double() - ro).abs().max().item(), dr.fa_tol(ro)
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float("-inf")).all()), what
    assert bool((o[~fin] == 0).all()), what  # a query that sees no key
    el = (lse.double()[fin] - rl[fin]).abs().max().item() if bool(fin.any()) else 0.0
    bl = dr.lse_tol(rl)
    print("%s: O err %.3e / bound %.3e = %.4f   LSE err %.3e / bound %.3e = %.4f" % (what, eo, bo, eo / bo, el, bl, el / bl))
    assert eo <= bo, (what, eo, bo)
    assert el <= bl, (what, el, bl)
    return fin


def fixed_T(qb, kp, vp, bt_row, n, dev="cuda"):
    """fa2_prefill_paged with B = 1, T = T_b on one sequence: (o [T,Hq,D], lse [T,Hq]) on the CPU."""
    import cuda_learn_notes_amd as pkg
    qd = qb[None].contiguous().to(dev)
    o = torch.full_like(qd, float("nan"))
    lse = torch.full(qd.shape[:3], float("nan"), dtype=torch.float32, device=dev)
    pkg.fa2_prefill_paged(qd, kp.to(dev), vp.to(dev), bt_row[None].contiguous().to(dev), torch.tensor([n], dtype=torch.int32, device=dev), o, lse)
    torch.cuda.synchronize()
    return o[0].cpu(), lse[0].cpu()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("ci", range(len(vr.CASES)), ids=CASE_IDS)
def test_parity_and_bit_equality_with_the_fixed_T_entry(built, dev, ci, D):
    """Per length vector: parity with the reference, and for every sequence with T_b >= 1 the bits of fa2_prefill_paged on that sequence alone."""
    geom, T = vr.CASES[ci]
    qs, k, v = problem(ci, D)
    q, cu = pack(qs)
    for kk in (0, 3, 5):
        lens = contexts(geom, T)(kk)
        kp, vp, bt = pr.make_pool(k, v, geom[2], lens, seed=kk)
        o, lse = run(q, kp, vp, bt, lens, cu)
        check(o, lse, q, kp, vp, bt, lens, cu, "D=%d %s T=%s lens=%s" % (D, geom, T, lens))
        for b, t in enumerate(T):
            if t:
                o1, l1 = fixed_T(qs[b], kp, vp, bt[b], lens[b])
                assert torch.equal(bits(o[cu[b]:cu[b + 1]]), bits(o1)) and torch.equal(fbits(lse[cu[b]:cu[b + 1]]), fbits(l1)), (D, geom, b, lens)
    nolse = run(q, kp, vp, bt, lens, cu, want_lse=False)
    assert torch.equal(bits(nolse[0]), bits(o))


@pytest.mark.parametrize("D", DS)
def test_sequences_shorter_than_their_chunk_and_empty_ones(built, dev, D):
    """len_b < T_b: the leading queries see nothing (O = 0, LSE = -inf exactly); len_b = 0: none does; a length past the capacity is clamped."""
    ci = 0
    geom, T = vr.CASES[ci]  # T = [40, 0, 1, 33, 130]
    qs, k, v = problem(ci, D)
    q, cu = pack(qs)
    lens = [7, 5, 0, 1 << 30, 100]  # 33 leading queries dead; T = 0; len = 0; clamped to 1024; 30 leading queries dead
    kp, vp, bt = pr.make_pool(k, v, geom[2], lens, seed=1)
    o, lse = run(q, kp, vp, bt, lens, cu)
    fin = check(o, lse, q, kp, vp, bt, lens, cu, "D=%d %s T=%s lens=%s" % (D, geom, T, lens))
    want = torch.cat([torch.arange(t) >= t - min(n, 1024) for t, n in zip(T, lens)])
    assert torch.equal(fin, want[:, None].expand_as(fin))
    for b in (0, 3, 4):
        o1, l1 = fixed_T(qs[b], kp, vp, bt[b], lens[b])
        assert torch.equal(bits(o[cu[b]:cu[b + 1]]), bits(o1)) and torch.equal(fbits(lse[cu[b]:cu[b + 1]]), fbits(l1)), (D, b)


@pytest.mark.parametrize("D", DS)
def test_a_sequence_does_not_depend_on_its_batch(built, dev, D):
    """Other neighbours with other T, another page placement and another position in the packed tensor: the same bits."""
    geom, T = vr.CASES[0]
    qs, k, v = problem(0, D)
    lens = contexts(geom, T)(2)
    q, cu = pack(qs)
    kp, vp, bt = pr.make_pool(k, v, geom[2], lens, seed=3)
    base = run(q, kp, vp, bt, lens, cu)
    check(base[0], base[1], q, kp, vp, bt, lens, cu, "batch D=%d lens=%s" % (D, lens))
    g = torch.Generator().manual_seed(77 + D)
    for b in (0, 3, 4):  # sequence b between other neighbours: [17 tokens, b, 129 tokens], reversed cache order, three rows in front
        qs2 = (torch.randn(17, geom[1], D, generator=g).half(), qs[b], torch.randn(129, geom[1], D, generator=g).half())
        k2, v2 = (torch.stack((x[(b + 1) % 5], x[b], x[(b + 2) % 5])) for x in (k, v))
        lens2 = [200, lens[b], 700]
        q2, cu2 = pack(qs2, first=3)
        kp2, vp2, bt2 = pr.make_pool(k2, v2, geom[2], lens2, seed=10 + b, extra=4)
        o2, l2 = run(q2, kp2, vp2, bt2, lens2, cu2)
        untouched(o2, l2, cu2)
        assert torch.equal(bits(o2[cu2[1]:cu2[2]]), bits(base[0][cu[b]:cu[b + 1]])), (D, b)
        assert torch.equal(fbits(l2[cu2[1]:cu2[2]]), fbits(base[1][cu[b]:cu[b + 1]])), (D, b)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("ci", [0, 2], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_rows_outside_the_sequences_are_not_touched(built, dev, ci, D):
    """Five spare rows behind cu_q[B], then cu_q[0] = 3 as well: out and lse keep their NaN bits there, and the sequences keep their bits. The
    spare rows of q hold 6e4: read into a product, they would show."""
    geom, T = vr.CASES[ci]
    qs, k, v = problem(ci, D)
    lens = contexts(geom, T)(1)
    kp, vp, bt = pr.make_pool(k, v, geom[2], lens, seed=2)
    q0, cu0 = pack(qs)
    q3, cu3 = pack(qs, first=3)
    a, b = run(q0, kp, vp, bt, lens, cu0), run(q3, kp, vp, bt, lens, cu3)
    check(a[0], a[1], q0, kp, vp, bt, lens, cu0, "D=%d %s cu[0]=0" % (D, geom))
    check(b[0], b[1], q3, kp, vp, bt, lens, cu3, "D=%d %s cu[0]=3" % (D, geom))
    assert torch.equal(bits(a[0][:cu0[-1]]), bits(b[0][3:cu3[-1]])) and torch.equal(fbits(a[1][:cu0[-1]]), fbits(b[1][3:cu3[-1]]))


@pytest.mark.parametrize("D", DS)
def test_calls_repeat_and_the_offsets_are_read_on_the_device(built, dev, D):
    import cuda_learn_notes_amd as pkg
    geom, T = vr.CASES[0]
    Hkv, G, page, mp = geom
    qs, k, v = problem(0, D)
    q, cu = pack(qs)
    T2 = [3, 129, 0, 64, 8]  # the same B and total_q, another split
    cu2 = vr.cu_of(T2)
    assert cu2[-1] == cu[-1]
    lens, lens2 = [700, 5, 1, 999, 333], [257, 129, 40, 1024, 8]
    kp, vp, bt = pr.make_pool(k, v, page, [page * mp] * len(T), seed=3)  # every page live: both length vectors are served by the same table
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    cd = torch.tensor(cu, dtype=torch.int32, device=dev)
    new = lambda: (torch.full_like(qd, float("nan")), torch.full(qd.shape[:2], float("nan"), dtype=torch.float32, device=dev))  # noqa: E731
    outs = [new() for _ in range(8)]
    for o, l in outs:
        pkg.fa2_prefill_paged_varlen(qd, kd, vd, bd, sl, cd, o, l)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(o), bits(outs[0][0])) and torch.equal(fbits(l), fbits(outs[0][1])) for o, l in outs[1:])
    check(outs[0][0].cpu(), outs[0][1].cpu(), q, kp, vp, bt, lens, cu, "first D=%d" % D)
    sl.copy_(torch.tensor(lens2, dtype=torch.int32)), cd.copy_(torch.tensor(cu2, dtype=torch.int32))  # in place: the same pointers
    o2, l2 = new()
    pkg.fa2_prefill_paged_varlen(qd, kd, vd, bd, sl, cd, o2, l2)
    torch.cuda.synchronize()
    fresh = run(q, kp, vp, bt, lens2, cu2)
    assert torch.equal(bits(o2.cpu()), bits(fresh[0])) and torch.equal(fbits(l2.cpu()), fbits(fresh[1]))
    assert not torch.equal(bits(o2), bits(outs[0][0]))
    check(fresh[0], fresh[1], q, kp, vp, bt, lens2, cu2, "changed in place D=%d" % D)


def append_step(ci, D, T, lens, seed):
    """(q packed, cu, k_new, v_new [total_q,Hkv,D], the pools before the append, the pools after it): the rows of the T_b newest tokens of dense
    caches, the full pool with those rows overwritten by -1, and the full pool. Every page is live, so one table serves any lengths."""
    (Hkv, G, page, mp), _ = vr.CASES[ci]
    g = torch.Generator().manual_seed(seed + D)
    qs = tuple(torch.randn(max(t, 0), Hkv * G, D, generator=g).half() for t in T)
    k, v = (torch.randn(len(T), Hkv, page * mp, D, generator=g).half() for _ in range(2))
    q, cu = pack(qs)
    kb, vb = k.clone(), v.clone()
    k_new, v_new = (torch.full((q.shape[0], Hkv, D), 6e4, dtype=torch.half) for _ in range(2))
    for b, t in enumerate(T):
        for i in range(t):
            pos = lens[b] - t + i
            if 0 <= pos < page * mp:
                k_new[cu[b] + i], v_new[cu[b] + i] = k[b, :, pos], v[b, :, pos]
                kb[b, :, pos], vb[b, :, pos] = -1.0, -1.0
    full = pr.make_pool(k, v, page, [page * mp] * len(T), seed=5)
    before = pr.make_pool(kb, vb, page, [page * mp] * len(T), seed=5)
    assert torch.equal(full[2], before[2]) and not torch.equal(bits(full[0]), bits(before[0]))
    return q, cu, k_new, v_new, before, full


@pytest.mark.parametrize("D", DS)
def test_graph_replay_of_append_and_prefill_reads_everything_from_the_device(built, dev, D):
    """kv_append_paged_varlen and fa2_prefill_paged_varlen captured on one stream; offsets, lengths, new rows, q and pools changed in place; the
    replay equals the eager pair on the same device state bit for bit, and the reference."""
    import cuda_learn_notes_amd as pkg
    T1, T2 = [40, 0, 1, 33, 130], [3, 129, 0, 64, 8]
    lens1, lens2 = [100, 9, 1024, 7, 130], [640, 129, 33, 1000, 8]  # the fourth sequence of the first step is shorter than its chunk
    first, second = append_step(0, D, T1, lens1, seed=2), append_step(0, D, T2, lens2, seed=3)
    q, cu, k_new, v_new, before, full = first
    qd, knd, vnd = (t.to(dev) for t in (q, k_new, v_new))
    kd, vd, bd = (t.to(dev) for t in before)
    sl = torch.tensor(lens1, dtype=torch.int32, device=dev)
    cd = torch.tensor(cu, dtype=torch.int32, device=dev)
    og = torch.full_like(qd, float("nan"))
    lg = torch.full(qd.shape[:2], float("nan"), dtype=torch.float32, device=dev)

    def step(kp, vp, o, lse):
        pkg.kv_append_paged_varlen(knd, vnd, kp, vp, bd, sl, cd)
        pkg.fa2_prefill_paged_varlen(qd, kp, vp, bd, sl, cd, o, lse)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(kd, vd, og, lg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(bits(kd.cpu()), bits(full[0])) and torch.equal(bits(vd.cpu()), bits(full[1]))
    check(og.cpu(), lg.cpu(), q, *full, lens1, cu, "eager pair D=%d lens=%s" % (D, lens1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(kd, vd, og, lg)
    q, cu, k_new, v_new, before, full = second
    sl.copy_(torch.tensor(lens2, dtype=torch.int32)), cd.copy_(torch.tensor(cu, dtype=torch.int32))
    qd.copy_(q), knd.copy_(k_new), vnd.copy_(v_new), kd.copy_(before[0]), vd.copy_(before[1])
    og.fill_(float("nan")), lg.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    ke, ve = before[0].to(dev), before[1].to(dev)
    oe, le = torch.full_like(qd, float("nan")), torch.full_like(lg, float("nan"))
    step(ke, ve, oe, le)
    torch.cuda.synchronize()
    assert torch.equal(bits(kd), bits(ke)) and torch.equal(bits(vd), bits(ve)) and torch.equal(bits(og), bits(oe)) and torch.equal(fbits(lg), fbits(le))
    assert torch.equal(bits(kd.cpu()), bits(full[0])) and torch.equal(bits(vd.cpu()), bits(full[1]))
    check(og.cpu(), lg.cpu(), q, *full, lens2, cu, "graph replay D=%d lens=%s" % (D, lens2))


def test_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    D = 64
    (Hkv, G, page, mp), T = vr.CASES[0]
    Hq, B = Hkv * G, len(T)
    qs, k, v = problem(0, D)
    q, cu = pack(qs)
    tq = q.shape[0]
    lens = [300, 0, 1000, 40, 555]
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    cd = torch.tensor(cu, dtype=torch.int32, device=dev)
    o = torch.empty_like(qd)
    f = pkg.fa2_prefill_paged_varlen
    f(qd, kd, vd, bd, sl, cd, o)
    q6 = torch.zeros(tq, 3, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="group size 3"):
        f(q6, kd, vd, bd, sl, cd, torch.empty_like(q6))
    kp48 = torch.zeros(8, Hkv, 48, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="page size 48"):
        f(qd, kp48, kp48.clone(), bd, sl, cd, o)
    q96, kp96 = torch.zeros(tq, Hq, 96, dtype=torch.half, device=dev), torch.zeros(8, Hkv, page, 96, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="headdim 96"):
        f(q96, kp96, kp96.clone(), bd, sl, cd, torch.empty_like(q96))
    with pytest.raises(RuntimeError, match="status -1"):  # out is an input
        f(qd, kd, vd, bd, sl, cd, qd)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):  # a cu_q of length B
        f(qd, kd, vd, bd, sl, cd[:B].contiguous(), o)
    with pytest.raises(RuntimeError, match="no CPU path"):  # cu_q on the CPU
        f(qd, kd, vd, bd, sl, cd.cpu(), o)
    bad = [
        lambda: f(qd.float(), kd, vd, bd, sl, cd, o),                                               # dtype
        lambda: f(qd, kd, vd, bd.long(), sl, cd, o),
        lambda: f(qd, kd, vd, bd, sl.long(), cd, o),
        lambda: f(qd, kd, vd, bd, sl, cd.long(), o),
        lambda: f(qd, kd, vd, bd, sl, cd, o, lse=torch.empty(tq, Hq, dtype=torch.half, device=dev)),
        lambda: f(qd[None], kd, vd, bd, sl, cd, o[None]),                                           # q with a batch dimension
        lambda: f(qd, kd, vd[:4].contiguous(), bd, sl, cd, o),                                      # shape
        lambda: f(qd, kd, vd, bd, sl[:1], cd, o),
        lambda: f(qd, kd, vd, bd, sl, cd, o[:2].contiguous()),
        lambda: f(qd, kd, vd, bd, sl, cd, o, lse=torch.empty(tq, dtype=torch.float32, device=dev)),
        lambda: f(qd, kd, vd, bd.cpu(), sl, cd, o),                                                 # table / lengths on the CPU
        lambda: f(qd, kd, vd, bd, sl.cpu(), cd, o),
        lambda: f(qd[::2], kd, vd, bd, sl, cd, o[::2]),                                             # not contiguous
    ]
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
