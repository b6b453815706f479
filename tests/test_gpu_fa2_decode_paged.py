"""GPU: decode attention over a paged KV cache with grouped query heads (cuda_learn_notes_amd.fa2_decode_paged, cln_fa2_decode_paged;
csrc/flash_attn_decode_paged.cuh) against the fp64 reference of tests/paged_decode_reference.py. Every case runs on a pool with more pages than
it needs, the live pages placed by a seeded permutation with the sequences interleaved, every page no live entry names filled with NaN and every
table entry past ceil(len / page) pointing at an in-range poison page of NaN (paged_decode_reference.make_pool): a kernel that follows a wrong
entry or reads a row too many gives a wrong number, not a fault. Every case prints its figures before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
from fa_reference import onehot_problem  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, Hkv, G, page, max_pages): chosen from the plan (paged_decode_reference.plan mirrors it; test_shapes_cover_the_plan asserts what they cover)
SHAPES = [(3, 2, 1, 16, 63), (2, 2, 4, 16, 64), (2, 1, 8, 128, 8), (1, 1, 2, 256, 32), (3, 5, 1, 32, 2), (1, 1, 8, 16, 1)]
DS = [64, 128]
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def plan_of(shape, D):
    B, Hkv, G, page, mp = shape
    return pr.plan(B, Hkv * G, Hkv, mp, page, D)


@functools.lru_cache(maxsize=None)
def problem(shape, D, seed=0):
    """Gaussian fp16 (q [B,Hq,D], dense k, v [B,Hkv,Nmax,D]) on the CPU, made once per shape and never modified."""
    B, Hkv, G, page, mp = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * Hkv + 17 * G + page * mp + D)
    q = torch.randn(B, Hkv * G, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, page * mp, D, generator=g).half() for _ in range(2))
    return q, k, v


def lengths_for(shape, D):
    B, Hkv, G, page, mp = shape
    S, C, _ = plan_of(shape, D)
    step, Nmax = dr.key_step(D), page * mp
    want = [1, 2, page - 1, page, page + 1, step - 1, step, step + 1, C - 1, C, C + 1, 2 * C + 1, Nmax - 1, Nmax]
    return sorted({n for n in want if 1 <= n <= Nmax})


def run(q, kp, vp, bt, lens, want_lse=True, workspace=None, dev="cuda"):
    import cuda_learn_notes_amd as pkg
    qd, kd, vd, bd = (t.to(dev) if not t.is_cuda else t for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full_like(qd, float("nan"))
    lse = torch.full(qd.shape[:2], float("nan"), dtype=torch.float32, device=dev) if want_lse else None
    pkg.fa2_decode_paged(qd, kd, vd, bd, sl, o, lse, workspace)
    torch.cuda.synchronize()
    return o.cpu(), (lse.cpu() if want_lse else None)


def check(o, lse, q, kp, vp, bt, lens, what):
    """O within fa_tol(ref), LSE within lse_tol(ref); returns the two ratios error / bound."""
    ro, rl = pr.ref_decode_paged(q, kp, vp, bt, lens)
    assert bool(torch.isfinite(o).all()), what
    eo, bo = (o.double() - ro).abs().max().item(), dr.fa_tol(ro)
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float("-inf")).all()), what
    el = (lse.double()[fin] - rl[fin]).abs().max().item() if bool(fin.any()) else 0.0
    bl = dr.lse_tol(rl)
    print("%s: O err %.3e / bound %.3e = %.4f   LSE err %.3e / bound %.3e = %.4f" % (what, eo, bo, eo / bo, el, bl, el / bl))
    assert eo <= bo, (what, eo, bo)
    assert el <= bl, (what, el, bl)
    return eo / bo, el / bl


def pool_run_check(shape, D, lens, what, seed=0):
    q, k, v = problem(shape, D)
    kp, vp, bt = pr.make_pool(k, v, shape[3], lens, seed=seed)
    o, lse = run(q, kp, vp, bt, lens)
    return (o, lse) + check(o, lse, q, kp, vp, bt, lens, what)


def test_shapes_cover_the_plan(built):
    for D in DS:
        step = dr.key_step(D)
        splits = [built.fa2_decode_paged_plan(B, Hkv * G, Hkv, mp, page, D)[0] for (B, Hkv, G, page, mp) in SHAPES]
        assert splits == [plan_of(s, D)[0] for s in SHAPES]
        assert any(s == 1 for s in splits) and any(s >= 3 for s in splits), (D, splits)
        assert {s[2] for s in SHAPES} == set(pr.GROUPS)
        assert any(s[3] < step for s in SHAPES) and any(s[3] > step for s in SHAPES), D
    assert max(s[3] * s[4] for s in SHAPES) <= 8192


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parity_at_the_plan_boundaries(built, dev, shape, D):
    B = shape[0]
    worst = (0.0, 0.0)
    for i, n in enumerate(lengths_for(shape, D)):
        r = pool_run_check(shape, D, [n] * B, "D=%d %s len=%d" % (D, shape, n), seed=i)[2:]
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("D=%d %s S=%d C=%d: worst error / bound  O %.4f  LSE %.4f" % ((D, shape) + plan_of(shape, D)[:2] + worst))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 2, 1, 16, 63), (3, 1, 4, 32, 32)], ids=ids)
def test_mixed_batch(built, dev, shape, D):
    """A length of 1, a length that leaves the last S - 1 splits empty, and Nmax, in one batch."""
    S, C, _ = plan_of(shape, D)
    assert S >= 3 and C - 3 > 1
    lens = [1, C - 3, shape[3] * shape[4]]
    pool_run_check(shape, D, lens, "D=%d %s lens=%s" % (D, shape, lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (2, 1, 8, 128, 8)], ids=ids)
def test_page_placement_does_not_change_a_bit(built, dev, shape, D):
    q, k, v = problem(shape, D)
    Nmax = shape[3] * shape[4]
    lens = [Nmax - 324, Nmax]
    pools = [pr.make_pool(k, v, shape[3], lens, **kw) for kw in (dict(order="identity"), dict(seed=1), dict(seed=2, extra=9))]
    assert not torch.equal(pools[0][2], pools[1][2]) and not torch.equal(pools[1][2], pools[2][2]) and pools[2][0].shape[0] > pools[1][0].shape[0]
    outs = [run(q, kp, vp, bt, lens) for (kp, vp, bt) in pools]
    check(outs[0][0], outs[0][1], q, *pools[0], lens, "identity order D=%d %s" % (D, shape))
    for o, lse in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (2, 1, 8, 128, 8), (3, 5, 1, 32, 2)], ids=ids)
def test_nothing_outside_the_live_rows_is_used(built, dev, shape, D):
    B, Hkv, G, page, mp = shape
    S, C, need = plan_of(shape, D)
    q, k, v = problem(shape, D)
    lens = [C + 1, page * mp - 1, 5][:B] if S > 1 else [page + 1, page * mp - 1, 5][:B]
    assert all(n % page for n in lens)  # every last live page has rows at or past the length
    plain_pool = pr.make_pool(k, v, page, lens)
    plain = run(q, *plain_pool, lens)
    for fill in (float("nan"), 6e4):
        kf, vf = k.clone(), v.clone()
        for b in range(B):
            kf[b, :, lens[b]:] = fill
            vf[b, :, lens[b]:] = fill
        kp, vp, bt = pr.make_pool(kf, vf, page, lens)
        assert torch.equal(bt, plain_pool[2])
        kd, vd = kp.to(dev), vp.to(dev)
        ws = torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device=dev)
        o, lse = run(q, kd, vd, bt, lens, workspace=ws)
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
        assert torch.equal(o, plain[0]) and torch.equal(lse, plain[1])
        # the caches are inputs: bit-unchanged (compared as integers, they hold NaN)
        assert torch.equal(kd.cpu().view(torch.int16), kp.view(torch.int16)) and torch.equal(vd.cpu().view(torch.int16), vp.view(torch.int16))
    check(plain[0], plain[1], q, *plain_pool, lens, "D=%d %s lens=%s" % (D, shape, lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (3, 2, 1, 16, 63), (3, 5, 1, 32, 2)], ids=ids)
def test_guard_bands(built, dev, shape, D):
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp = shape
    Hq, Nmax = Hkv * G, page * mp
    S, C, need = pkg.fa2_decode_paged_plan(B, Hq, Hkv, mp, page, D)
    q, k, v = problem(shape, D)
    lens = [Nmax, 1, Nmax // 2][:B]
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    GB = 256
    ob = torch.full((B * Hq * D + 2 * GB,), 777.0, dtype=torch.half, device=dev)
    lb = torch.full((B * Hq + 2 * GB,), 777.0, dtype=torch.float32, device=dev)
    wb = torch.full((need + 2 * GB,), 0xA5, dtype=torch.uint8, device=dev)
    o, lse, ws = ob[GB:GB + B * Hq * D].view(B, Hq, D), lb[GB:GB + B * Hq].view(B, Hq), wb[GB:GB + need]
    assert ws.numel() == need
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    pkg.fa2_decode_paged(q.to(dev), kp.to(dev), vp.to(dev), bt.to(dev), sl, o, lse, ws if need else None)
    torch.cuda.synchronize()
    for buf, n in ((ob, B * Hq * D), (lb, B * Hq)):
        assert bool((buf[:GB] == 777.0).all()) and bool((buf[GB + n:] == 777.0).all())
    assert bool((wb[:GB] == 0xA5).all()) and bool((wb[GB + need:] == 0xA5).all())
    check(o.cpu(), lse.cpu(), q, kp, vp, bt, lens, "guarded D=%d %s" % (D, shape))


@pytest.mark.parametrize("D", DS)
def test_one_hot_keys_select_one_value_row(built, dev, D):
    N, page, G = 4096, 16, 2  # (1, 1, ...): the plan splits the keys 16 ways
    assert pr.plan(1, G, 1, N // page, page, D)[0] >= 3
    _, k, v, _, _ = onehot_problem(N, D, False, seed=5)
    bits = (N - 1).bit_length()
    score = 16.0 * (D // bits) * bits / D ** 0.5
    kd, vd = k.view(1, 1, N, D), v.view(1, 1, N, D)
    for n, ts in ((N, (0, N - 1)), (3000, (2999, 1234)), (257, (256, 17))):
        kp, vp, bt = pr.make_pool(kd, vd, page, [n], seed=n)
        q = torch.stack([k[t] * 16 for t in ts]).view(1, G, D)  # the two heads of the group select different keys
        o, lse = run(q, kp, vp, bt, [n])
        for h, t in enumerate(ts):
            assert torch.equal(o[0, h], v[t]), (D, n, t)
            assert abs(lse[0, h].item() - score) <= 1e-5 * score, (D, n, t, lse[0, h].item(), score)


@pytest.mark.parametrize("D", DS)
def test_constant_values_zero_query_and_single_key(built, dev, D):
    shape = (3, 1, 4, 32, 32)
    B, Hkv, G, page, mp = shape
    q, k, v = problem(shape, D)
    lens = [1000, 385, 77]
    # constant V: every accumulator sums at most a few dozen terms c p in fp32, relative error ~1e-6, far below half an fp16 ulp of c
    kp, vp, bt = pr.make_pool(k, torch.full_like(v, 0.375), page, lens)
    o, _ = run(q, kp, vp, bt, lens)
    assert bool((o == 0.375).all())
    # q = 0: the mean of the live rows, LSE = ln(len)
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    o, lse = run(torch.zeros_like(q), kp, vp, bt, lens)
    for b in range(B):
        mean = v[b, :, :lens[b]].double().mean(dim=1).repeat_interleave(G, dim=0)
        assert (o[b].double() - mean).abs().max().item() <= dr.fa_tol(mean), (D, b)
        ln = torch.log(torch.tensor(float(lens[b]), dtype=torch.float64)).item()
        assert (lse[b].double() - ln).abs().max().item() <= 1e-6 * ln, (D, b, lse[b], ln)
    # one key: O = V[0] bit for bit for every head of a group; LSE = q . K_0 / sqrt(D), an fp32 dot product of D exact products
    # (error <= (D + 4) 2^-24 sum|q_i k_i| / sqrt(D))
    kp, vp, bt = pr.make_pool(k, v, page, [1] * B)
    o, lse = run(q, kp, vp, bt, [1] * B)
    k0, v0 = k[:, :, 0].repeat_interleave(G, dim=1), v[:, :, 0].repeat_interleave(G, dim=1)
    assert torch.equal(o, v0)
    s = (q.double() * k0.double()).sum(-1) / D ** 0.5
    bound = (D + 4) * 2.0 ** -24 * (q.double() * k0.double()).abs().sum(-1) / D ** 0.5
    assert bool(((lse.double() - s).abs() <= bound).all()), (D, (lse.double() - s).abs().max().item(), bound.min().item())


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (2, 1, 8, 128, 8), (1, 1, 8, 16, 1)], ids=ids)
def test_heads_of_a_group_are_independent_and_equal_queries_give_equal_bits(built, dev, shape, D):
    B, Hkv, G, page, mp = shape
    q, k, v = problem(shape, D)
    lens = [page * mp - 3, page * mp // 2 + 1][:B]
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    kd, vd, bd = kp.to(dev), vp.to(dev), bt.to(dev)
    base = run(q, kd, vd, bd, lens)
    q2 = q.clone()
    q2[:, 1::G] = problem(shape, D, seed=1)[0][:, 1::G]  # head 1 of every group
    other = run(q2, kd, vd, bd, lens)
    keep = [h for h in range(Hkv * G) if h % G != 1]
    assert torch.equal(base[0][:, keep], other[0][:, keep]) and torch.equal(base[1][:, keep], other[1][:, keep])
    assert not torch.equal(base[0][:, 1::G], other[0][:, 1::G])
    qe = q[:, ::G].repeat_interleave(G, dim=1)  # all G queries of a group equal
    o, lse = run(qe, kd, vd, bd, lens)
    o, lse = o.view(B, Hkv, G, D), lse.view(B, Hkv, G)
    assert all(torch.equal(o[:, :, h], o[:, :, 0]) and torch.equal(lse[:, :, h], lse[:, :, 0]) for h in range(G))
    assert torch.equal(o[:, :, 0], base[0][:, ::G])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 2, 1, 16, 63), (2, 1, 8, 128, 8), (3, 5, 1, 32, 2)], ids=ids)
def test_lengths_are_clamped(built, dev, shape, D):
    B, Hkv, G, page, mp = shape
    Nmax = page * mp
    q, k, v = problem(shape, D)
    kp, vp, bt = pr.make_pool(k, v, page, [Nmax] * B)
    kd, vd, bd = kp.to(dev), vp.to(dev), bt.to(dev)
    o, lse = run(q, kd, vd, bd, [0, -3, 0][:B])
    assert bool((o == 0).all()) and bool((lse == float("-inf")).all())
    full = run(q, kd, vd, bd, [Nmax] * B)
    over = run(q, kd, vd, bd, [Nmax + 7] * B)
    assert torch.equal(full[0], over[0]) and torch.equal(full[1], over[1])
    mixed = run(q, kd, vd, bd, [0, Nmax + 7, -3][:B])
    assert bool((mixed[0][0] == 0).all()) and torch.equal(mixed[0][1], full[0][1]) and torch.equal(mixed[1][1], full[1][1])
    assert mixed[1][0].tolist() == [float("-inf")] * (Hkv * G)
    check(full[0], full[1], q, kp, vp, bt, [Nmax] * B, "full D=%d %s" % (D, shape))


@pytest.mark.parametrize("D", DS)
def test_a_sequence_does_not_depend_on_its_neighbours_and_calls_repeat(built, dev, D):
    import cuda_learn_notes_amd as pkg
    shape = (3, 1, 4, 32, 32)
    B, Hkv, G, page, mp = shape
    q, k, v = problem(shape, D)
    lens = [700, 999, 333]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=3)
    first = run(q, kp, vp, bt, lens)
    # other lengths, other data and other pages for sequences 0 and 2; sequence 1 keeps its logical rows but moves in the pool
    k2, v2 = (t.clone() for t in problem(shape, D, seed=1)[1:])
    k2[1], v2[1] = k[1], v[1]
    lens2 = [1, 999, 1024]
    kp2, vp2, bt2 = pr.make_pool(k2, v2, page, lens2, seed=4)
    other = run(q, kp2, vp2, bt2, lens2)
    assert not torch.equal(bt[1], bt2[1])
    assert torch.equal(first[0][1], other[0][1]) and torch.equal(first[1][1], other[1][1])
    assert not torch.equal(first[0][0], other[0][0])
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    ws = torch.empty(max(pkg.fa2_decode_paged_plan(B, Hkv * G, Hkv, mp, page, D)[2], 16), dtype=torch.uint8, device=dev)
    outs = [(torch.empty_like(qd), torch.empty(B, Hkv * G, dtype=torch.float32, device=dev)) for _ in range(20)]
    for o, l in outs:
        pkg.fa2_decode_paged(qd, kd, vd, bd, sl, o, l, ws)
    torch.cuda.synchronize()
    assert all(torch.equal(o.cpu(), first[0]) and torch.equal(l.cpu(), first[1]) for o, l in outs)


@pytest.mark.parametrize("D", DS)
def test_agrees_with_the_dense_decode_at_group_size_one(built, dev, D):
    import cuda_learn_notes_amd as pkg
    shape = (3, 2, 1, 16, 63)
    B, Hkv, G, page, mp = shape
    q, k, v = problem(shape, D)
    lens = [1008, 385, 77]
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    o, lse = run(q, kp, vp, bt, lens)
    kg, vg = pr.gather(kp, bt, lens), pr.gather(vp, bt, lens)  # the gathered dense cache: zero where nothing is live
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    od, ld = torch.empty_like(q, device=dev), torch.empty(B, Hkv, dtype=torch.float32, device=dev)
    pkg.fa2_decode(q.to(dev), kg.to(dev), vg.to(dev), sl, od, ld)
    torch.cuda.synchronize()
    ro, rl = pr.ref_decode_paged(q, kp, vp, bt, lens)
    err, lerr = (o.float() - od.cpu().float()).abs().max().item(), (lse - ld.cpu()).abs().max().item()
    print("D=%d: paged vs dense decode O %.3e (bound %.3e)  LSE %.3e (bound %.3e)" % (D, err, 2 * dr.fa_tol(ro), lerr, 2 * dr.lse_tol(rl)))
    assert err <= 2 * dr.fa_tol(ro) and lerr <= 2 * dr.lse_tol(rl)  # two different plans: each within its own bound of the reference


@pytest.mark.parametrize("D", DS)
def test_graph_replay_reads_table_lengths_and_cache_from_the_device(built, dev, D):
    import cuda_learn_notes_amd as pkg
    shape = (2, 2, 4, 16, 64)
    B, Hkv, G, page, mp = shape
    Hq, Nmax = Hkv * G, page * mp
    S, C, need = pkg.fa2_decode_paged_plan(B, Hq, Hkv, mp, page, D)
    assert S > 1  # two kernels in a line
    q, k, v = problem(shape, D)
    # both pools hold every page of both sequences: what changes between capture and replay is where the table points and the lengths
    kp, vp, bt = pr.make_pool(k, v, page, [Nmax] * B, seed=1)
    qd, kd, vd, bd = (t.to(dev).clone() for t in (q, kp, vp, bt))
    sl = torch.tensor([100, Nmax], dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    og, lg = torch.zeros_like(qd), torch.zeros(B, Hq, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pkg.fa2_decode_paged(qd, kd, vd, bd, sl, og, lg, ws)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pkg.fa2_decode_paged(qd, kd, vd, bd, sl, og, lg, ws)
    # on the device: other lengths, the pool and the table of another permutation, and one live K row rewritten
    lens2 = [900, 513]
    kp2, vp2, bt2 = pr.make_pool(k, v, page, [Nmax] * B, seed=2)
    assert kp2.shape == kp.shape and not torch.equal(bt2, bt)
    g = torch.Generator().manual_seed(5)
    kp2[int(bt2[0, 899 // page]), 1, 899 % page] = torch.randn(D, generator=g).half() * 4
    sl.copy_(torch.tensor(lens2, dtype=torch.int32))
    kd.copy_(kp2), vd.copy_(vp2), bd.copy_(bt2)
    og.zero_(), lg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    oe, le = torch.empty_like(qd), torch.empty_like(lg)
    pkg.fa2_decode_paged(qd, kd, vd, bd, sl, oe, le)
    torch.cuda.synchronize()
    assert torch.equal(og, oe) and torch.equal(lg, le)
    check(og.cpu(), lg.cpu(), q, kp2, vp2, bt2, lens2, "graph replay D=%d" % D)


def test_python_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp, D = 2, 2, 4, 16, 64, 64
    Hq, P = Hkv * G, 200
    q = torch.zeros(B, Hq, D, dtype=torch.half, device=dev)
    kp = torch.zeros(P, Hkv, page, D, dtype=torch.half, device=dev)
    vp = torch.zeros_like(kp)
    bt = torch.zeros(B, mp, dtype=torch.int32, device=dev)
    sl = torch.tensor([5, 9], dtype=torch.int32, device=dev)
    o = torch.empty_like(q)
    f = pkg.fa2_decode_paged
    need = pkg.fa2_decode_paged_plan(B, Hq, Hkv, mp, page, D)[2]
    assert need > 0
    bad = [
        lambda: f(q.float(), kp, vp, bt, sl, o),                                              # dtype
        lambda: f(q, kp.float(), vp, bt, sl, o),
        lambda: f(q, kp, vp, bt.long(), sl, o),
        lambda: f(q, kp, vp, bt, sl.long(), o),
        lambda: f(q, kp, vp, bt, sl, o, lse=torch.empty(B, Hq, dtype=torch.half, device=dev)),
        lambda: f(q, kp, vp[:100].contiguous(), bt, sl, o),                                   # shape
        lambda: f(q, kp, vp, bt[:1], sl, o),
        lambda: f(q, kp, vp, bt.view(-1), sl, o),
        lambda: f(q, kp, vp, bt, sl[:1], o),
        lambda: f(q, kp, vp, bt, sl, o[:, :4].contiguous()),
        lambda: f(q, kp, vp, bt, sl, o, lse=torch.empty(B, Hq + 1, dtype=torch.float32, device=dev)),
        lambda: f(q.unsqueeze(2), kp, vp, bt, sl, o),
        lambda: f(q, kp[:, :, :, :32].contiguous(), vp[:, :, :, :32].contiguous(), bt, sl, o),    # D of the pages
        lambda: f(q, kp, vp, bt.cpu(), sl, o),                                                # table / lengths on the CPU
        lambda: f(q, kp, vp, bt, sl.cpu(), o),
        lambda: f(q, kp, vp, bt, sl, o, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev)),  # short workspace
    ]
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
    kp3 = torch.zeros(P, 3, page, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="no multiple"):  # Hq % Hkv != 0
        f(q, kp3, kp3.clone(), bt, sl, o)
    q6 = torch.zeros(B, 6, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="group size 3"):
        f(q6, kp, vp, bt, sl, torch.empty_like(q6))
    kp48 = torch.zeros(P, Hkv, 48, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="page size 48"):
        f(q, kp48, kp48.clone(), bt, sl, o)
    q96, kp96 = torch.zeros(B, Hq, 96, dtype=torch.half, device=dev), torch.zeros(P, Hkv, page, 96, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="headdim 96"):
        f(q96, kp96, kp96.clone(), bt, sl, torch.empty_like(q96))
