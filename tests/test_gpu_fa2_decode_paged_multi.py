"""GPU: multi-token decode attention over a paged KV cache with grouped query heads (cuda_learn_notes_amd.fa2_decode_paged_multi,
cln_fa2_decode_paged_multi; csrc/flash_attn_decode_paged_multi.cuh) against the fp64 reference of tests/multi_decode_reference.py. Every case runs
on a pool of paged_decode_reference.make_pool: more pages than needed, the live pages placed by a seeded permutation with the sequences
interleaved, every page no live entry names filled with NaN and every table entry past ceil(len / page) pointing at an in-range poison page of NaN
-- a kernel that follows a wrong entry or reads a row too many gives a wrong number, not a fault. Tolerances: decode_reference.fa_tol / lse_tol;
-inf LSE entries are compared exactly. Every case prints its figures before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import multi_decode_reference as mr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, Hkv, G, page, max_pages, T): chosen from the plan (multi_decode_reference.plan mirrors it; test_shapes_cover_the_plan asserts what they cover)
SHAPES = [(2, 1, 1, 16, 63, 3), (1, 2, 2, 32, 40, 5), (1, 1, 8, 256, 4, 3), (1, 1, 8, 16, 48, 8), (2, 1, 4, 64, 3, 2), (1, 2, 4, 128, 2, 1),
          (1, 1, 8, 16, 12, 5)]
MIXED = (3, 1, 4, 32, 32, 5)  # S = 4, C = 256, R = 20: two row tiles, the second one partly empty
DS = [64, 128]
STEP = mr.KEY_STEP
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def plan_of(shape, D):
    B, Hkv, G, page, mp, T = shape
    return mr.plan(B, T, Hkv * G, Hkv, mp, page, D)


@functools.lru_cache(maxsize=None)
def problem(shape, D, seed=0):
    """Gaussian fp16 (q [B,T,Hq,D], dense k, v [B,Hkv,Nmax,D]) on the CPU, made once per shape and never modified."""
    B, Hkv, G, page, mp, T = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * Hkv + 17 * G + page * mp + D + 31 * T)
    q = torch.randn(B, T, Hkv * G, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, page * mp, D, generator=g).half() for _ in range(2))
    return q, k, v


def lengths_for(shape, D):
    B, Hkv, G, page, mp, T = shape
    S, C, _ = plan_of(shape, D)
    Nmax = page * mp
    want = [1, T - 1, T, T + 1, page - 1, page, page + 1, STEP, STEP + 1, C, C + 1, C + T - 1, 2 * C + 1, Nmax - 1, Nmax]
    return sorted({n for n in want if 1 <= n <= Nmax})


def run(q, kp, vp, bt, lens, want_lse=True, workspace=None, dev="cuda"):
    import cuda_learn_notes_amd as pkg
    qd, kd, vd, bd = (t.to(dev) if not t.is_cuda else t for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full_like(qd, float("nan"))
    lse = torch.full(qd.shape[:3], float("nan"), dtype=torch.float32, device=dev) if want_lse else None
    pkg.fa2_decode_paged_multi(qd, kd, vd, bd, sl, o, lse, workspace)
    torch.cuda.synchronize()
    return o.cpu(), (lse.cpu() if want_lse else None)


def check(o, lse, q, kp, vp, bt, lens, what):
    """O within fa_tol(ref), LSE within lse_tol(ref), -inf LSE entries exactly; returns the two ratios error / bound."""
    ro, rl = mr.ref_decode_paged_multi(q, kp, vp, bt, lens)
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
    return eo / bo, el / bl


def pool_run_check(shape, D, lens, what, seed=0):
    q, k, v = problem(shape, D)
    kp, vp, bt = pr.make_pool(k, v, shape[3], lens, seed=seed)
    o, lse = run(q, kp, vp, bt, lens)
    return (o, lse) + check(o, lse, q, kp, vp, bt, lens, what)


def test_shapes_cover_the_plan(built):
    for D in DS:
        splits = [built.fa2_decode_paged_multi_plan(B, T, Hkv * G, Hkv, mp, page, D)[0] for (B, Hkv, G, page, mp, T) in SHAPES]
        assert splits == [plan_of(s, D)[0] for s in SHAPES]
        assert any(s == 1 for s in splits) and any(s >= 3 for s in splits), (D, splits)
    assert {s[2] for s in SHAPES} == set(pr.GROUPS)
    assert {s[5] for s in SHAPES} >= {1, 2, 3, 5, 8}
    assert {s[5] * s[2] for s in SHAPES} >= {3, 10, 24, 64}
    assert any(s[3] < STEP for s in SHAPES) and any(s[3] > STEP for s in SHAPES)
    assert max(s[3] * s[4] for s in SHAPES + [MIXED]) <= 8192
    S, C, _ = plan_of(MIXED, 64)
    assert S >= 3 and MIXED[5] >= 3 and plan_of(MIXED, 128)[:2] == (S, C)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parity_at_the_plan_and_mask_boundaries(built, dev, shape, D):
    B = shape[0]
    worst = (0.0, 0.0)
    for i, n in enumerate(lengths_for(shape, D)):
        r = pool_run_check(shape, D, [n] * B, "D=%d %s len=%d" % (D, shape, n), seed=i)[2:]
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("D=%d %s S=%d C=%d: worst error / bound  O %.4f  LSE %.4f" % ((D, shape) + plan_of(shape, D)[:2] + worst))


@pytest.mark.parametrize("D", DS)
def test_mixed_batch(built, dev, D):
    """Length 1 (< T: queries with no key), C + 1 (the second split holds one key, which only the last query sees) and Nmax, in one batch."""
    S, C, _ = plan_of(MIXED, D)
    lens = [1, C + 1, MIXED[3] * MIXED[4]]
    o, lse, _, _ = pool_run_check(MIXED, D, lens, "D=%d %s lens=%s" % (D, MIXED, lens))
    T = MIXED[5]
    assert bool((lse[0, :T - 1] == float("-inf")).all()) and bool(torch.isfinite(lse[0, T - 1]).all()) and bool(torch.isfinite(lse[1:]).all())


@pytest.mark.parametrize("D", DS)
def test_empty_sequence(built, dev, D):
    T = MIXED[5]
    lens = [MIXED[3] * MIXED[4] - 7, 0, T + 40]
    o, lse, _, _ = pool_run_check(MIXED, D, lens, "D=%d %s lens=%s" % (D, MIXED, lens))
    assert bool((o[1] == 0).all()) and bool((lse[1] == float("-inf")).all())
    assert bool(torch.isfinite(lse[0]).all()) and bool(torch.isfinite(lse[2]).all()) and bool((o[0] != 0).any()) and bool((o[2] != 0).any())


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [MIXED, (1, 1, 8, 16, 48, 8), (1, 1, 8, 16, 12, 5)], ids=ids)
def test_causal_tail_is_masked_not_down_weighted(built, dev, shape, D):
    """For every t < T - 1: the K and V rows [n(b,t), len_b), which later queries see and query t must not, overwritten with 6e4 -- row t of O and
    LSE keeps its bits. The lengths put the causal edge across a split, a page and a key tile boundary at once."""
    B, Hkv, G, page, mp, T = shape
    S, C, _ = plan_of(shape, D)
    Nmax = page * mp
    lens = [min(C + 2, Nmax), min(2 * C + 1, Nmax - 3), STEP + 1][:B] if S > 1 else [STEP + 2]
    q, k, v = problem(shape, D)
    pool = pr.make_pool(k, v, page, lens)
    clean = run(q, *pool, lens)
    check(clean[0], clean[1], q, *pool, lens, "clean D=%d %s lens=%s" % (D, shape, lens))
    for t in range(T - 1):
        kf, vf = k.clone(), v.clone()
        for b in range(B):
            n_bt = max(lens[b] - (T - 1 - t), 0)
            kf[b, :, n_bt:lens[b]] = 6e4
            vf[b, :, n_bt:lens[b]] = 6e4
        kp, vp, bt = pr.make_pool(kf, vf, page, lens)
        assert torch.equal(bt, pool[2])
        o, lse = run(q, kp, vp, bt, lens)
        assert torch.equal(o[:, t], clean[0][:, t]) and torch.equal(lse[:, t], clean[1][:, t]), (D, shape, t)
        assert torch.equal(o[:, :t], clean[0][:, :t]) and torch.equal(lse[:, :t], clean[1][:, :t]), (D, shape, t)  # the rows before it see even less


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [MIXED, (1, 2, 2, 32, 40, 5), (2, 1, 4, 64, 3, 2)], ids=ids)
def test_nothing_outside_the_live_rows_is_used(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
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
        o, lse = run(q, kd, vd, bt, lens)
        assert bool(torch.isfinite(o).all())
        assert torch.equal(o, plain[0]) and torch.equal(lse, plain[1])
        # the caches are inputs: bit-unchanged (compared as integers, they hold NaN)
        assert torch.equal(kd.cpu().view(torch.int16), kp.view(torch.int16)) and torch.equal(vd.cpu().view(torch.int16), vp.view(torch.int16))
    check(plain[0], plain[1], q, *plain_pool, lens, "D=%d %s lens=%s" % (D, shape, lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(1, 2, 2, 32, 40, 5), (1, 1, 8, 256, 4, 3)], ids=ids)
def test_page_placement_does_not_change_a_bit(built, dev, shape, D):
    q, k, v = problem(shape, D)
    Nmax = shape[3] * shape[4]
    lens = [Nmax - 324]
    pools = [pr.make_pool(k, v, shape[3], lens, **kw) for kw in (dict(order="identity"), dict(seed=1), dict(seed=2, extra=9))]
    assert not torch.equal(pools[0][2], pools[1][2]) and not torch.equal(pools[1][2], pools[2][2]) and pools[2][0].shape[0] > pools[1][0].shape[0]
    outs = [run(q, kp, vp, bt, lens) for (kp, vp, bt) in pools]
    check(outs[0][0], outs[0][1], q, *pools[0], lens, "identity order D=%d %s" % (D, shape))
    for o, lse in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1])


@pytest.mark.parametrize("D", DS)
def test_a_sequence_does_not_depend_on_its_batch(built, dev, D):
    B, Hkv, G, page, mp, T = MIXED
    q, k, v = problem(MIXED, D)
    lens = [700, 999, 3]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=3)
    batch = run(q, kp, vp, bt, lens)
    check(batch[0], batch[1], q, kp, vp, bt, lens, "batch D=%d lens=%s" % (D, lens))
    for b in range(B):  # other queries, other caches, other lengths and other pages around sequence b
        lens2 = [1024 if i != b else lens[b] for i in range(B)]
        q2, k2, v2 = (t.clone() for t in problem(MIXED, D, seed=1))
        q2[b], k2[b], v2[b] = q[b], k[b], v[b]
        kp2, vp2, bt2 = pr.make_pool(k2, v2, page, lens2, seed=4 + b)
        other = run(q2, kp2, vp2, bt2, lens2)
        assert torch.equal(batch[0][b], other[0][b]) and torch.equal(batch[1][b], other[1][b]), (D, b)
    # alone: B = 1 has the plan of B = 3 here (the mirror says so), so the bits can be compared
    assert plan_of((1,) + MIXED[1:], D)[:2] == plan_of(MIXED, D)[:2]
    for b in range(B):
        kp1, vp1, bt1 = pr.make_pool(k[b:b + 1], v[b:b + 1], page, lens[b:b + 1], seed=9)
        o1, l1 = run(q[b:b + 1].contiguous(), kp1, vp1, bt1, lens[b:b + 1])
        assert torch.equal(o1[0], batch[0][b]) and torch.equal(l1[0], batch[1][b]), (D, b)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 1, 4, 32, 32, 1), (1, 2, 4, 128, 2, 1)], ids=ids)
def test_one_token_agrees_with_the_single_query_kernel(built, dev, shape, D):
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp, T = shape
    assert T == 1
    q, k, v = problem(shape, D)
    lens = [page * mp - 16, 385, 77][:B]
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    o, lse = run(q, kp, vp, bt, lens)
    ro, rl = mr.ref_decode_paged_multi(q, kp, vp, bt, lens)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    o1 = torch.empty(B, Hkv * G, D, dtype=torch.half, device=dev)
    l1 = torch.empty(B, Hkv * G, dtype=torch.float32, device=dev)
    pkg.fa2_decode_paged(q[:, 0].contiguous().to(dev), kp.to(dev), vp.to(dev), bt.to(dev), sl, o1, l1)
    torch.cuda.synchronize()
    err, lerr = (o[:, 0].float() - o1.cpu().float()).abs().max().item(), (lse[:, 0] - l1.cpu()).abs().max().item()
    print("D=%d %s: multi (T = 1) vs fa2_decode_paged  O %.3e (bound %.3e)  LSE %.3e (bound %.3e)" % (D, shape, err, dr.fa_tol(ro), lerr, dr.lse_tol(rl)))
    assert err <= dr.fa_tol(ro) and lerr <= dr.lse_tol(rl)
    check(o, lse, q, kp, vp, bt, lens, "T=1 D=%d %s" % (D, shape))


@pytest.mark.parametrize("D", DS)
def test_calls_repeat_and_the_lengths_are_read_on_the_device(built, dev, D):
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp, T = MIXED
    Hq = Hkv * G
    q, k, v = problem(MIXED, D)
    lens, lens2 = [700, 999, 333], [257, 3, 1024]
    kp, vp, bt = pr.make_pool(k, v, page, [page * mp] * B, seed=3)  # every page live: both length vectors are served by the same table
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    ws = torch.empty(max(pkg.fa2_decode_paged_multi_plan(B, T, Hq, Hkv, mp, page, D)[2], 16), dtype=torch.uint8, device=dev)
    outs = [(torch.empty_like(qd), torch.empty(B, T, Hq, dtype=torch.float32, device=dev)) for _ in range(8)]
    for o, l in outs:
        pkg.fa2_decode_paged_multi(qd, kd, vd, bd, sl, o, l, ws)
    torch.cuda.synchronize()
    assert all(torch.equal(o, outs[0][0]) and torch.equal(l, outs[0][1]) for o, l in outs[1:])
    check(outs[0][0].cpu(), outs[0][1].cpu(), q, kp, vp, bt, lens, "first D=%d lens=%s" % (D, lens))
    sl.copy_(torch.tensor(lens2, dtype=torch.int32))  # in place: the same pointer, other lengths
    o2, l2 = torch.empty_like(qd), torch.empty(B, T, Hq, dtype=torch.float32, device=dev)
    pkg.fa2_decode_paged_multi(qd, kd, vd, bd, sl, o2, l2, ws)
    torch.cuda.synchronize()
    fresh = run(q, kd, vd, bd, lens2)
    assert torch.equal(o2.cpu(), fresh[0]) and torch.equal(l2.cpu(), fresh[1])
    assert not torch.equal(o2, outs[0][0])
    check(fresh[0], fresh[1], q, kp, vp, bt, lens2, "changed in place D=%d lens=%s" % (D, lens2))


def test_workspace_and_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    D = 64
    B, Hkv, G, page, mp, T = MIXED
    Hq = Hkv * G
    S, C, need = pkg.fa2_decode_paged_multi_plan(B, T, Hq, Hkv, mp, page, D)
    assert S > 1 and need == B * T * Hq * S * (D + 2) * 4
    q, k, v = problem(MIXED, D)
    lens = [C + 1, 1000, 2]
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    base = run(q, kp, vp, bt, lens)
    ws = torch.full((need // 4 + 64,), float("nan"), dtype=torch.float32, device=dev)
    mine = run(q, kp, vp, bt, lens, workspace=ws)
    assert torch.equal(base[0], mine[0]) and torch.equal(base[1], mine[1])
    assert bool(torch.isnan(ws[need // 4:]).all())  # nothing written behind the plan's bytes
    nolse = run(q, kp, vp, bt, lens, want_lse=False)
    assert torch.equal(nolse[0], base[0])
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    o = torch.empty_like(qd)
    f = pkg.fa2_decode_paged_multi
    with pytest.raises(RuntimeError, match="workspace of %d bytes, the plan needs %d" % (need - 1, need)):
        f(qd, kd, vd, bd, sl, o, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    q9 = torch.zeros(B, 9, Hq, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match=r"T 9 not supported \(1 … 8\)"):
        f(q9, kd, vd, bd, sl, torch.empty_like(q9))
    q6 = torch.zeros(B, T, 3, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="group size 3"):
        f(q6, kd, vd, bd, sl, torch.empty_like(q6))
    kp48 = torch.zeros(8, Hkv, 48, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="page size 48"):
        f(qd, kp48, kp48.clone(), bd, sl, o)
    q96, kp96 = torch.zeros(B, T, Hq, 96, dtype=torch.half, device=dev), torch.zeros(8, Hkv, page, 96, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="headdim 96"):
        f(q96, kp96, kp96.clone(), bd, sl, torch.empty_like(q96))
    bad = [
        lambda: f(qd.float(), kd, vd, bd, sl, o),                                                # dtype
        lambda: f(qd, kd, vd, bd.long(), sl, o),
        lambda: f(qd, kd, vd, bd, sl.long(), o),
        lambda: f(qd, kd, vd, bd, sl, o, lse=torch.empty(B, T, Hq, dtype=torch.half, device=dev)),
        lambda: f(qd[:, 0].contiguous(), kd, vd, bd, sl, o[:, 0].contiguous()),                  # q without the T dimension
        lambda: f(qd, kd, vd[:4].contiguous(), bd, sl, o),                                       # shape
        lambda: f(qd, kd, vd, bd, sl[:1], o),
        lambda: f(qd, kd, vd, bd, sl, o[:, :2].contiguous()),
        lambda: f(qd, kd, vd, bd, sl, o, lse=torch.empty(B, Hq, dtype=torch.float32, device=dev)),
        lambda: f(qd, kd, vd, bd.cpu(), sl, o),                                                  # table / lengths on the CPU
        lambda: f(qd, kd, vd, bd, sl.cpu(), o),
    ]
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
