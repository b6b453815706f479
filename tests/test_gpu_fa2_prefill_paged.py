"""GPU: prefill attention (any T) over a paged KV cache with grouped query heads (cuda_learn_notes_amd.fa2_prefill_paged, cln_fa2_prefill_paged;
csrc/flash_attn_prefill_paged.cuh) against the fp64 reference of tests/prefill_reference.py. Every case runs on a pool of
paged_decode_reference.make_pool: more pages than needed, the live pages placed by a seeded permutation with the sequences interleaved, every page
no live entry names filled with NaN and every table entry past ceil(len / page) pointing at an in-range poison page of NaN -- a kernel that follows
a wrong entry or reads a row too many gives a wrong number, not a fault. Tolerances: decode_reference.fa_tol / lse_tol; -inf LSE entries and the
zero rows of O are compared exactly. The boundaries come from prefill_reference.ROW_TILE / KEY_STEP, which the describe text is checked against.
Every case prints its figures before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import prefill_reference as pf  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, Hkv, G, page, max_pages, T)
SHAPES = [(1, 1, 1, 16, 24, 9), (1, 1, 8, 16, 20, 17), (2, 2, 4, 64, 8, 33), (1, 1, 2, 256, 2, 200), (1, 2, 1, 32, 40, 130), (1, 1, 8, 128, 4, 64)]
MIXED = (3, 1, 4, 32, 32, 40)  # R = 160: a whole workgroup tile and a quarter of one
DS = [64, 128]
ROWS, STEP = pf.ROW_TILE, pf.KEY_STEP
ids = lambda s: "x".join(map(str, s))  # noqa: E731
bits = lambda t: t.view(torch.int16)  # noqa: E731


@functools.lru_cache(maxsize=None)
def problem(shape, D, seed=0):
    """Gaussian fp16 (q [B,T,Hq,D], dense k, v [B,Hkv,Nmax,D]) on the CPU, made once per shape and never modified."""
    B, Hkv, G, page, mp, T = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * Hkv + 17 * G + page * mp + D + 31 * T)
    q = torch.randn(B, T, Hkv * G, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, page * mp, D, generator=g).half() for _ in range(2))
    return q, k, v


def lengths_for(shape):
    B, Hkv, G, page, mp, T = shape
    Nmax = page * mp
    want = [1, T - 1, T, T + 1, page - 1, page, page + 1, STEP, STEP + 1, ROWS // G + STEP - 1, Nmax - 1, Nmax]
    return sorted({min(max(n, 1), Nmax) for n in want})


def run(q, kp, vp, bt, lens, want_lse=True, dev="cuda"):
    import cuda_learn_notes_amd as pkg
    qd, kd, vd, bd = (t.to(dev) if not t.is_cuda else t for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full_like(qd, float("nan"))
    lse = torch.full(qd.shape[:3], float("nan"), dtype=torch.float32, device=dev) if want_lse else None
    pkg.fa2_prefill_paged(qd, kd, vd, bd, sl, o, lse)
    torch.cuda.synchronize()
    return o.cpu(), (lse.cpu() if want_lse else None)


def check(o, lse, q, kp, vp, bt, lens, what):
    """O within fa_tol(ref), LSE within lse_tol(ref), -inf LSE entries and their zero rows exactly; returns the two ratios error / bound."""
    ro, rl = pf.ref_prefill_paged(q, kp, vp, bt, lens)
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


def test_shapes_cover(built):
    R = [s[5] * s[2] for s in SHAPES]
    assert any(r < pf.MFMA_ROWS for r in R)                                     # below one MFMA tile
    assert any(s[5] * s[2] == ROWS + s[2] for s in SHAPES)                      # one whole workgroup tile plus exactly one token
    assert any(r % ROWS == 0 for r in R) and any(r >= 3 * ROWS for r in R)      # exact multiples; many tiles
    assert any(r % pf.MFMA_ROWS and r % pf.WAVE_ROWS for r in R)                # a last MFMA tile and a last wave that are partly empty
    assert {s[2] for s in SHAPES} == set(pr.GROUPS)
    assert any(s[3] < STEP for s in SHAPES) and any(s[3] == STEP for s in SHAPES) and any(s[3] > STEP for s in SHAPES)
    assert max(s[3] * s[4] for s in SHAPES + [MIXED]) <= 1280
    assert MIXED[0] >= 3 and ROWS < MIXED[5] * MIXED[2] < 2 * ROWS
    for s in SHAPES + [MIXED]:  # the constants above are the kernel's
        B, Hkv, G, page, mp, T = s
        t = built.manifest.describe_prefill_paged(B, T, Hkv * G, Hkv, mp, page, 128)
        assert " rows=%d keys=%d:" % (ROWS, STEP) in t and "%d workgroups" % (B * Hkv * pf.tiles(T, G)) in t, t


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parity_at_the_tile_page_and_mask_boundaries(built, dev, shape, D):
    B = shape[0]
    worst = (0.0, 0.0)
    for i, n in enumerate(lengths_for(shape)):
        r = pool_run_check(shape, D, [n] * B, "D=%d %s len=%d" % (D, shape, n), seed=i)[2:]
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("D=%d %s: worst error / bound  O %.4f  LSE %.4f" % ((D, shape) + worst))


@pytest.mark.parametrize("D", DS)
def test_mixed_batch(built, dev, D):
    """A ragged prefill batch: length 1 (< T: only the last query is live, right-aligned), a mid value whose first queries see nothing, and Nmax."""
    B, Hkv, G, page, mp, T = MIXED
    lens = [1, T - 7, page * mp]
    o, lse, _, _ = pool_run_check(MIXED, D, lens, "D=%d %s lens=%s" % (D, MIXED, lens))
    assert bool((lse[0, :T - 1] == float("-inf")).all()) and bool(torch.isfinite(lse[0, T - 1]).all())
    assert bool((lse[1, :7] == float("-inf")).all()) and bool(torch.isfinite(lse[1, 7:]).all()) and bool(torch.isfinite(lse[2]).all())


@pytest.mark.parametrize("D", DS)
def test_empty_sequence(built, dev, D):
    T = MIXED[5]
    lens = [MIXED[3] * MIXED[4] - 7, 0, T + 40]
    o, lse, _, _ = pool_run_check(MIXED, D, lens, "D=%d %s lens=%s" % (D, MIXED, lens))
    assert bool((o[1] == 0).all()) and bool((lse[1] == float("-inf")).all())
    assert bool(torch.isfinite(lse[0]).all()) and bool(torch.isfinite(lse[2]).all()) and bool((o[0] != 0).any()) and bool((o[2] != 0).any())


def edge_tokens(T, G):
    """The tokens of the first and last row of every workgroup tile and of every 16-row MFMA tile, without the last token (nothing lies behind
    its causal edge)."""
    R = T * G
    rows = {r for r0 in range(0, R, pf.MFMA_ROWS) for r in (r0, min(r0 + pf.MFMA_ROWS, R) - 1)}
    rows |= {r for r0 in range(0, R, ROWS) for r in (r0, min(r0 + ROWS, R) - 1)}
    return sorted({r // G for r in rows} - {T - 1})


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(1, 1, 8, 16, 20, 17), (2, 2, 4, 64, 8, 33), (1, 2, 1, 32, 40, 130)], ids=ids)
def test_causal_tail_is_masked_not_down_weighted(built, dev, shape, D):
    """For the tokens t at the edges of the row tiles: the K and V rows [n(b,t), len_b), which later queries see and query t must not, overwritten
    with 6e4 -- the rows <= t of O and LSE keep their bits. The lengths put the causal edges across key step and page boundaries."""
    B, Hkv, G, page, mp, T = shape
    Nmax = page * mp
    lens = [min(STEP + T // 2 + 1, Nmax), Nmax - 3][:B]
    assert all(n >= T for n in lens)
    q, k, v = problem(shape, D)
    pool = pr.make_pool(k, v, page, lens)
    clean = run(q, *pool, lens)
    check(clean[0], clean[1], q, *pool, lens, "clean D=%d %s lens=%s" % (D, shape, lens))
    ts = edge_tokens(T, G)
    assert 0 in ts and T - 2 in ts and (ROWS - 1) // G in ts and ROWS // G in ts + [T - 1]
    for t in ts:
        kf, vf = k.clone(), v.clone()
        for b in range(B):
            n_bt = lens[b] - (T - 1 - t)
            kf[b, :, n_bt:lens[b]] = 6e4
            vf[b, :, n_bt:lens[b]] = 6e4
        kp, vp, bt = pr.make_pool(kf, vf, page, lens)
        assert torch.equal(bt, pool[2])
        o, lse = run(q, kp, vp, bt, lens)
        assert torch.equal(o[:, :t + 1], clean[0][:, :t + 1]) and torch.equal(lse[:, :t + 1], clean[1][:, :t + 1]), (D, shape, t)
        assert not torch.equal(o[:, t + 1:], clean[0][:, t + 1:])  # the rows behind it do see the change


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [MIXED, (1, 2, 1, 32, 40, 130), (2, 2, 4, 64, 8, 33)], ids=ids)
def test_nothing_outside_the_live_rows_is_used(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    q, k, v = problem(shape, D)
    lens = [page + 1, page * mp - 1, 5][:B]
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
        assert torch.equal(bits(kd.cpu()), bits(kp)) and torch.equal(bits(vd.cpu()), bits(vp))
    check(plain[0], plain[1], q, *plain_pool, lens, "D=%d %s lens=%s" % (D, shape, lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(1, 2, 1, 32, 40, 130), (1, 1, 2, 256, 2, 200)], ids=ids)
def test_page_placement_does_not_change_a_bit(built, dev, shape, D):
    q, k, v = problem(shape, D)
    Nmax = shape[3] * shape[4]
    lens = [Nmax - 100]
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
    for b in range(B):  # alone
        kp1, vp1, bt1 = pr.make_pool(k[b:b + 1], v[b:b + 1], page, lens[b:b + 1], seed=9)
        o1, l1 = run(q[b:b + 1].contiguous(), kp1, vp1, bt1, lens[b:b + 1])
        assert torch.equal(o1[0], batch[0][b]) and torch.equal(l1[0], batch[1][b]), (D, b)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 1, 4, 32, 32, 1), (3, 1, 4, 32, 32, 5), (1, 2, 2, 16, 24, 8), (1, 1, 8, 128, 4, 8)], ids=ids)
def test_few_tokens_agree_with_the_multi_token_decode_kernel(built, dev, shape, D):
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp, T = shape
    assert T <= 8
    q, k, v = problem(shape, D)
    lens = [page * mp - 16, 385, 3][:B]
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    o, lse = run(q, kp, vp, bt, lens)
    ro, rl = pf.ref_prefill_paged(q, kp, vp, bt, lens)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    o1 = torch.empty(B, T, Hkv * G, D, dtype=torch.half, device=dev)
    l1 = torch.empty(B, T, Hkv * G, dtype=torch.float32, device=dev)
    pkg.fa2_decode_paged_multi(q.to(dev), kp.to(dev), vp.to(dev), bt.to(dev), sl, o1, l1)
    torch.cuda.synchronize()
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(l1.cpu()), fin) and torch.equal(torch.isfinite(lse), fin)
    err, lerr = (o.float() - o1.cpu().float()).abs().max().item(), (lse[fin] - l1.cpu()[fin]).abs().max().item()
    print("D=%d %s: prefill vs fa2_decode_paged_multi  O %.3e (bound %.3e)  LSE %.3e (bound %.3e)" % (D, shape, err, dr.fa_tol(ro), lerr, dr.lse_tol(rl)))
    assert err <= dr.fa_tol(ro) and lerr <= dr.lse_tol(rl)
    check(o, lse, q, kp, vp, bt, lens, "T=%d D=%d %s" % (T, D, shape))


@pytest.mark.parametrize("D", DS)
def test_whole_prompt_agrees_with_the_dense_causal_kernel(built, dev, D):
    """G = 1, len = T = 256 on an identity pool: the shape fa2_fwd_causal serves too."""
    import cuda_learn_notes_amd as pkg
    shape = (2, 2, 1, 64, 4, 256)
    B, H, G, page, mp, T = shape
    q, k, v = problem(shape, D)
    lens = [T] * B
    kp, vp, bt = pr.make_pool(k, v, page, lens, order="identity")
    o, lse = run(q, kp, vp, bt, lens)
    ro, _ = pf.ref_prefill_paged(q, kp, vp, bt, lens)
    qd = q.transpose(1, 2).contiguous().to(dev)  # [B,H,N,D]
    od = torch.empty_like(qd)
    pkg.fa2_fwd_causal(qd, k.to(dev), v.to(dev), od)
    torch.cuda.synchronize()
    err = (o.float() - od.cpu().transpose(1, 2).float()).abs().max().item()
    print("D=%d %s: prefill vs fa2_fwd_causal  O %.3e (bound %.3e)" % (D, shape, err, dr.fa_tol(ro)))
    assert err <= dr.fa_tol(ro)
    check(o, lse, q, kp, vp, bt, lens, "dense D=%d %s" % (D, shape))


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
    outs = [(torch.empty_like(qd), torch.empty(B, T, Hq, dtype=torch.float32, device=dev)) for _ in range(8)]
    for o, l in outs:
        pkg.fa2_prefill_paged(qd, kd, vd, bd, sl, o, l)
    torch.cuda.synchronize()
    assert all(torch.equal(o, outs[0][0]) and torch.equal(l, outs[0][1]) for o, l in outs[1:])
    check(outs[0][0].cpu(), outs[0][1].cpu(), q, kp, vp, bt, lens, "first D=%d lens=%s" % (D, lens))
    sl.copy_(torch.tensor(lens2, dtype=torch.int32))  # in place: the same pointer, other lengths
    o2, l2 = torch.empty_like(qd), torch.empty(B, T, Hq, dtype=torch.float32, device=dev)
    pkg.fa2_prefill_paged(qd, kd, vd, bd, sl, o2, l2)
    torch.cuda.synchronize()
    fresh = run(q, kd, vd, bd, lens2)
    assert torch.equal(o2.cpu(), fresh[0]) and torch.equal(l2.cpu(), fresh[1])
    assert not torch.equal(o2, outs[0][0])
    check(fresh[0], fresh[1], q, kp, vp, bt, lens2, "changed in place D=%d lens=%s" % (D, lens2))


def append_step(shape, D, lens, seed):
    """(k_new, v_new [B,T,Hkv,D], the pools before the append, the pools after it, the table): the rows of the T newest tokens of dense caches,
    the full pool with those rows overwritten by -1, and the full pool. Every page is live, so one table serves any lengths."""
    B, Hkv, G, page, mp, T = shape
    q, k, v = problem(shape, D, seed=seed)
    Nmax = page * mp
    kb, vb = k.clone(), v.clone()
    k_new, v_new = torch.zeros(B, T, Hkv, D, dtype=torch.half), torch.zeros(B, T, Hkv, D, dtype=torch.half)
    for b in range(B):
        for t in range(T):
            pos = lens[b] - T + t
            if 0 <= pos < Nmax:
                k_new[b, t], v_new[b, t] = k[b, :, pos], v[b, :, pos]
                kb[b, :, pos], vb[b, :, pos] = -1.0, -1.0
    full = pr.make_pool(k, v, page, [Nmax] * B, seed=5)
    before = pr.make_pool(kb, vb, page, [Nmax] * B, seed=5)
    assert torch.equal(full[2], before[2]) and not torch.equal(bits(full[0]), bits(before[0]))
    return q, k_new, v_new, before, full


@pytest.mark.parametrize("D", DS)
def test_graph_replay_of_append_and_prefill_reads_everything_from_the_device(built, dev, D):
    """kv_append_paged and fa2_prefill_paged captured on one stream; lengths, new rows, q and pools changed in place; the replay equals the eager
    pair on the same device state bit for bit, and the reference."""
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp, T = MIXED
    lens1, lens2 = [100, 1024, 7], [640, 33, 1000]  # the third sequence of the first step is shorter than the chunk
    first, second = append_step(MIXED, D, lens1, seed=2), append_step(MIXED, D, lens2, seed=3)
    q, k_new, v_new, before, full = first
    qd, knd, vnd = (t.to(dev) for t in (q, k_new, v_new))
    kd, vd, bd = (t.to(dev) for t in before)
    sl = torch.tensor(lens1, dtype=torch.int32, device=dev)
    og = torch.zeros_like(qd)
    lg = torch.zeros(B, T, Hkv * G, dtype=torch.float32, device=dev)

    def step(kp, vp, o, lse):
        pkg.kv_append_paged(knd, vnd, kp, vp, bd, sl)
        pkg.fa2_prefill_paged(qd, kp, vp, bd, sl, o, lse)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(kd, vd, og, lg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(bits(kd.cpu()), bits(full[0])) and torch.equal(bits(vd.cpu()), bits(full[1]))
    check(og.cpu(), lg.cpu(), q, *full, lens1, "eager pair D=%d lens=%s" % (D, lens1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(kd, vd, og, lg)
    q, k_new, v_new, before, full = second
    sl.copy_(torch.tensor(lens2, dtype=torch.int32))
    qd.copy_(q), knd.copy_(k_new), vnd.copy_(v_new), kd.copy_(before[0]), vd.copy_(before[1])
    og.zero_(), lg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    ke, ve = before[0].to(dev), before[1].to(dev)
    oe, le = torch.empty_like(qd), torch.empty_like(lg)
    step(ke, ve, oe, le)
    torch.cuda.synchronize()
    assert torch.equal(bits(kd), bits(ke)) and torch.equal(bits(vd), bits(ve)) and torch.equal(og, oe) and torch.equal(lg, le)
    assert torch.equal(bits(kd.cpu()), bits(full[0])) and torch.equal(bits(vd.cpu()), bits(full[1]))
    check(og.cpu(), lg.cpu(), q, *full, lens2, "graph replay D=%d lens=%s" % (D, lens2))


def test_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    D = 64
    B, Hkv, G, page, mp, T = MIXED
    Hq = Hkv * G
    q, k, v = problem(MIXED, D)
    lens = [300, 1000, 2]
    kp, vp, bt = pr.make_pool(k, v, page, lens)
    base = run(q, kp, vp, bt, lens)
    nolse = run(q, kp, vp, bt, lens, want_lse=False)
    assert torch.equal(nolse[0], base[0])
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    o = torch.empty_like(qd)
    f = pkg.fa2_prefill_paged
    q6 = torch.zeros(B, T, 3, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="group size 3"):
        f(q6, kd, vd, bd, sl, torch.empty_like(q6))
    kp48 = torch.zeros(8, Hkv, 48, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="page size 48"):
        f(qd, kp48, kp48.clone(), bd, sl, o)
    q96, kp96 = torch.zeros(B, T, Hq, 96, dtype=torch.half, device=dev), torch.zeros(8, Hkv, page, 96, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="headdim 96"):
        f(q96, kp96, kp96.clone(), bd, sl, torch.empty_like(q96))
    with pytest.raises(RuntimeError, match="status -1"):  # o is an input
        f(qd, kd, vd, bd, sl, qd)
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
        lambda: f(qd[:, ::2], kd, vd, bd, sl, o[:, ::2]),                                        # not contiguous
    ]
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
