"""GPU: the bf16 paged KV-cache append (cuda_learn_notes_amd.kv_append_paged_varlen_bf16, csrc/kv_append_paged_varlen_bf16.cuh) against the CPU
reference of tests/kv_append_bf16_reference.py -- copied rows bit for bit, rotated elements within its derived bound -- and one whole serving
step, append then attention, captured in a graph and replayed on changed device state. Pools come from paged_decode_reference.make_pool (NaN
poison pages, shuffled placement) and are compared as int16; the packed tensors carry rows in front of cu_q[0] and behind cu_q[B], filled with
2^100 (inputs) and a bit pattern (q_out), which the call must neither read nor write."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_append_bf16_reference as ar  # noqa: E402
import multi_decode_reference as mr  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import prefill_varlen_reference as vr  # noqa: E402
import test_gpu_paged_bf16_attention as at  # noqa: E402  (its helpers: check, bits, the fill patterns)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DS = [64, 128]
MODE_NAMES = ("none", "half", "interleaved")
CASE_IDS = ["x".join(map(str, g)) for g, _ in vr.CASES]
FIRST, SPARE = 3, 5
Q_FILL = at.O_FILL
bits, fbits = at.bits, at.fbits


@functools.lru_cache(maxsize=None)
def problem(ci, D, scale=1.0):
    """bf16 packed (k_new, v_new [total_q,Hkv,D], q [total_q,Hq,D]) with 2^100 in the rows outside the sequences, the offsets, and the dense k, v
    [B,Hkv,Nmax,D] the pools are cut from; on the CPU, made once and never modified."""
    (Hkv, G, page, mp), T = vr.CASES[ci]
    g = torch.Generator().manual_seed(31 * ci + D)
    cu = vr.cu_of(T, FIRST)
    tq = cu[-1] + SPARE
    k_new, v_new, q = ((torch.randn(tq, H, D, generator=g) * scale).to(BF) for H in (Hkv, Hkv, Hkv * G))
    for t in (k_new, v_new, q):
        t[t == 0] = 1.0
        t[:FIRST], t[cu[-1]:] = 2.0 ** 100, 2.0 ** 100
    k, v = (torch.randn(len(T), Hkv, page * mp, D, generator=g).to(BF) for _ in range(2))
    return k_new, v_new, q, tuple(cu), k, v


@functools.lru_cache(maxsize=None)
def random_table(max_pos, D):
    """Uniform in [-1, 1], not real sines: a wrong row or column of the table gives a wrong number."""
    return torch.rand(max_pos, D, generator=torch.Generator().manual_seed(max_pos + D)) * 2 - 1


def run(k_new, v_new, kp, vp, bt, lens, cu, q=None, table=None, rope="none", inplace=False, dev="cuda"):
    """The call on copies of everything; returns the pools and q_out on the CPU, after asserting that the inputs kept their bits."""
    import cuda_learn_notes_amd as pkg
    knd, vnd, kd, vd, bd = (t.to(dev) for t in (k_new, v_new, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    qd = qo = td = None
    if q is not None:
        qd = q.to(dev)
        qo = qd if inplace else torch.full(qd.shape, Q_FILL, dtype=torch.int16, device=dev).view(BF)
    if table is not None:
        td = table.to(dev)
    pkg.kv_append_paged_varlen_bf16(knd, vnd, kd, vd, bd, sl, cd, qd, qo, td, rope)
    torch.cuda.synchronize()
    assert torch.equal(bits(knd.cpu()), bits(k_new)) and torch.equal(bits(vnd.cpu()), bits(v_new))
    assert torch.equal(bd.cpu(), bt) and sl.cpu().tolist() == list(lens) and cd.cpu().tolist() == list(cu)
    if q is not None and not inplace:
        assert torch.equal(bits(qd.cpu()), bits(q))
    return kd.cpu(), vd.cpu(), (qo.cpu() if qo is not None else None)


def check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q, table, mode, page, what):
    """V and every K row no live token owns bit for bit (so every other byte of both pools is unchanged); the live K rows and q_out within the
    bound (mode 0: exact); the q_out rows of dead tokens zero; the rows of no sequence keep the pattern q_out was filled with."""
    rk, rv, k_live, rows, dead = ar.ref_append_varlen(k_new, v_new, kp, vp, bt, lens, cu, q, table, mode)
    assert torch.equal(bits(gv), bits(rv)), what
    keep = ~k_live[:, None, :, None].expand_as(gk)
    assert torch.equal(bits(gk)[keep], bits(kp)[keep]) and torch.equal(bits(gv)[keep], bits(vp)[keep]), what
    worst = 0.0
    for (row, b, pos, k_rot, k_mag, q_rot, q_mag) in rows:
        got = gk[int(bt[b, pos // page]), :, pos % page]
        assert bool(torch.isfinite(got).all()), what
        if mode == 0:
            assert torch.equal(got.double(), k_rot), what
        else:
            worst = max(worst, ((got.double() - k_rot).abs() / ar.bound(k_rot, k_mag)).max().item())
            if qo is not None:
                worst = max(worst, ((qo[row].double() - q_rot).abs() / ar.bound(q_rot, q_mag)).max().item())
    if qo is not None:
        outside = torch.cat((bits(qo[:cu[0]]), bits(qo[cu[-1]:])))
        assert bool((outside == Q_FILL).all()), what
        assert bool(torch.isfinite(qo[cu[0]:cu[-1]]).all()), what
        for row in dead:
            assert bool((bits(qo[row]) == 0).all()), (what, row)
    print("%s: worst error / bound %.4f over %d live and %d dead tokens" % (what, worst, len(rows), len(dead)))
    assert worst <= 1.0, (what, worst)
    return rows, dead


def lengths(geom, T):
    """One run from position 0, runs that start on the last row of a page, one that ends on the last row of the last page."""
    _, _, page, mp = geom
    Nmax = page * mp
    want = list(T)
    if len(T) > 1:
        want[-1] = Nmax
    for b in range(1, len(T) - 1):
        want[b] = min(page * b - 1 + T[b], Nmax)
    return want


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("ci", range(len(vr.CASES)), ids=CASE_IDS)
def test_append_every_token_live(built, dev, ci, mode, D):
    """The token counts of CASES x rope x with and without q, and q_out is q; V rows and all rope = none rows bit-equal to the inputs."""
    geom, T = vr.CASES[ci]
    page, Nmax = geom[2], geom[2] * geom[3]
    k_new, v_new, q, cu, k, v = problem(ci, D)
    lens = lengths(geom, T)
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=ci)
    what = "append D=%d %s %s" % (D, CASE_IDS[ci], MODE_NAMES[mode])
    if mode == 0:
        gk, gv, _ = run(k_new, v_new, kp, vp, bt, lens, cu)
        rows, dead = check_reference(gk, gv, None, k_new, v_new, kp, vp, bt, lens, cu, None, None, 0, page, what)
        assert len(rows) == sum(T) and not dead and not torch.equal(bits(gk), bits(kp))
        return
    table = random_table(Nmax, D)
    gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, cu, q, table, MODE_NAMES[mode])
    rows, dead = check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q, table, mode, page, what)
    assert len(rows) == sum(T) and not dead
    ak, av, none = run(k_new, v_new, kp, vp, bt, lens, cu, None, table, MODE_NAMES[mode])  # K alone: no q rows in the grid
    assert none is None and torch.equal(bits(ak), bits(gk)) and torch.equal(bits(av), bits(gv))
    ik, iv, iq = run(k_new, v_new, kp, vp, bt, lens, cu, q, table, MODE_NAMES[mode], inplace=True)  # q_out is q
    assert torch.equal(bits(ik), bits(gk)) and torch.equal(bits(iv), bits(gv))
    assert torch.equal(bits(iq[cu[0]:cu[-1]]), bits(qo[cu[0]:cu[-1]])) and not torch.equal(bits(iq[cu[0]:cu[-1]]), bits(q[cu[0]:cu[-1]]))
    assert torch.equal(bits(iq[:cu[0]]), bits(q[:cu[0]])) and torch.equal(bits(iq[cu[-1]:]), bits(q[cu[-1]:]))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_append_dead_tokens_write_nothing(built, dev, mode, D):
    """T = [40, 0, 1, 33, 130] on 1024 rows of cache with a table of 1000 rows: pos < 0 (7 of 40 live), a T_b = 0 sequence with a length, len = 0,
    pos >= max_pos (1000 .. 1009 of the run 977 .. 1009, with a rotation) and pos >= max_pages page (len = 1024 + 30). Every table entry that no
    live token resolves through lies outside [0, P)."""
    ci = 0
    geom, T = vr.CASES[ci]
    page, Nmax = geom[2], geom[2] * geom[3]
    k_new, v_new, q, cu, k, v = problem(ci, D)
    lens = [7, 77, 0, 1010, Nmax + 30]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=2)
    table = random_table(Nmax, D)[:1000].contiguous() if mode else None
    max_pos = 1000 if mode else Nmax
    used = torch.zeros(bt.shape, dtype=torch.bool)
    for b, t in enumerate(T):
        for i in range(t):
            pos = lens[b] - t + i
            if 0 <= pos < min(Nmax, max_pos):
                used[b, pos // page] = True
    bt = bt.clone()
    bt[~used] = torch.where(torch.arange(int((~used).sum())) % 2 == 0, -1, kp.shape[0] + 7).to(torch.int32)
    assert int((~used).sum()) > 0
    args = (q, table, MODE_NAMES[mode]) if mode else ()
    gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, cu, *args)
    rows, dead = check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q if mode else None, table, mode, page,
                                 "append D=%d dead tokens %s" % (D, MODE_NAMES[mode]))
    live4 = 76 if mode else 100  # positions 924 .. 1023 of the run 924 .. 1053, of them 924 .. 999 below max_pos
    live3 = 23 if mode else 33   # 977 .. 999 below max_pos
    assert len(rows) == 7 + live3 + live4 and len(dead) == sum(T) - len(rows)
    assert [r[0] for r in rows][:7] == list(range(cu[0] + 33, cu[0] + 40))


@pytest.mark.parametrize("D", DS)
def test_append_range_rows_at_two_to_the_17(built, dev, D):
    """k_new and v_new of magnitude 2^17 with rope = half: no fp16 can hold them; the pool rows are finite and within the bound."""
    ci = 2
    geom, T = vr.CASES[ci]
    page, Nmax = geom[2], geom[2] * geom[3]
    k_new, v_new, q, cu, k, v = problem(ci, D, 2.0 ** 17)
    assert float(k_new[cu[0]:cu[-1]].float().abs().max()) > 65504.0 and float(v_new[cu[0]:cu[-1]].float().abs().max()) > 65504.0
    lens = lengths(geom, T)
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=4)
    table = random_table(Nmax, D)
    gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, cu, q, table, "half")
    rows, _ = check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q, table, 1, page, "append range D=%d" % D)
    assert max(float(gk[int(bt[b, pos // page]), :, pos % page].float().abs().max()) for (_, b, pos, *_rest) in rows) > 65504.0


def test_append_repeats_its_bits(built, dev):
    geom, T = vr.CASES[0]
    k_new, v_new, q, cu, k, v = problem(0, 128)
    lens = lengths(geom, T)
    kp, vp, bt = pr.make_pool(k, v, geom[2], lens, seed=1)
    table = random_table(geom[2] * geom[3], 128)
    a, b = (run(k_new, v_new, kp, vp, bt, lens, cu, q, table, "interleaved") for _ in range(2))
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- one serving step, captured


def step_state(geom, T, lens, D, seed, spare=SPARE):
    """The state of one serving step on the CPU: packed q, cu, k_new, v_new [total_q,...], the pools before the append (the rows of the new tokens
    hold -1) and after it. Every page is live, so P is the same for every step of a geometry; the placement follows `seed`."""
    Hkv, G, page, mp = geom
    g = torch.Generator().manual_seed(seed + D)
    qs = tuple(torch.randn(t, Hkv * G, D, generator=g).to(BF) for t in T)
    k, v = (torch.randn(len(T), Hkv, page * mp, D, generator=g).to(BF) for _ in range(2))
    q, cu = at.pack(qs, first=0, spare=spare)
    kb, vb = k.clone(), v.clone()
    k_new, v_new = (torch.full((q.shape[0], Hkv, D), 2.0 ** 100, dtype=BF) for _ in range(2))
    for b, t in enumerate(T):
        for i in range(t):
            pos = lens[b] - t + i
            if 0 <= pos < page * mp:
                k_new[cu[b] + i], v_new[cu[b] + i] = k[b, :, pos], v[b, :, pos]
                kb[b, :, pos], vb[b, :, pos] = -1.0, -1.0
    full = pr.make_pool(k, v, page, [page * mp] * len(T), seed=seed)
    before = pr.make_pool(kb, vb, page, [page * mp] * len(T), seed=seed)
    assert torch.equal(full[2], before[2]) and not torch.equal(bits(full[0]), bits(before[0]))
    return dict(q=q, cu=cu, k_new=k_new, v_new=v_new, before=before, full=full, lens=lens)


def captured_step(dev, states, attend, reference):
    """Append + attention captured on one stream from states[0], then replayed on every later state (offsets, lengths, new rows, q, pools AND the
    table changed in place): each replay equals the eager pair on the same device state bit for bit, and the reference within the bound."""
    import cuda_learn_notes_amd as pkg
    s0 = states[0]
    qd, knd, vnd = (s0[x].to(dev) for x in ("q", "k_new", "v_new"))
    kd, vd, bd = (t.to(dev) for t in s0["before"])
    sl = torch.tensor(s0["lens"], dtype=torch.int32, device=dev)
    cd = torch.tensor(s0["cu"], dtype=torch.int32, device=dev)
    og = torch.zeros_like(qd)
    lg = torch.zeros(qd.shape[:2], dtype=torch.float32, device=dev)

    def step(kp, vp, o, lse):
        pkg.kv_append_paged_varlen_bf16(knd, vnd, kp, vp, bd, sl, cd)
        attend(pkg, qd, kp, vp, bd, sl, cd, o, lse)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(kd, vd, og, lg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(kd, vd, og, lg)
    for i, s in enumerate(states[1:]):
        assert not torch.equal(s["before"][2], bd.cpu()) and s["before"][0].shape == kd.shape  # another table, the same pool size
        sl.copy_(torch.tensor(s["lens"], dtype=torch.int32)), cd.copy_(torch.tensor(s["cu"], dtype=torch.int32))
        qd.copy_(s["q"]), knd.copy_(s["k_new"]), vnd.copy_(s["v_new"]), kd.copy_(s["before"][0]), vd.copy_(s["before"][1]), bd.copy_(s["before"][2])
        og.fill_(float("nan")), lg.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        ke, ve = s["before"][0].to(dev), s["before"][1].to(dev)
        oe, le = torch.full_like(og, float("nan")), torch.full_like(lg, float("nan"))
        step(ke, ve, oe, le)
        torch.cuda.synchronize()
        assert torch.equal(bits(kd), bits(ke)) and torch.equal(bits(vd), bits(ve)) and torch.equal(bits(og), bits(oe)) and torch.equal(fbits(lg), fbits(le))
        assert torch.equal(bits(kd.cpu()), bits(s["full"][0])) and torch.equal(bits(vd.cpu()), bits(s["full"][1]))
        reference(og.cpu(), lg.cpu(), s, "replay %d" % (i + 1))


@pytest.mark.parametrize("D", DS)
def test_graph_replay_of_append_and_prefill(built, dev, D):
    geom = vr.CASES[0][0]
    Ts = ([40, 0, 1, 33, 130], [3, 129, 0, 64, 8], [100, 1, 2, 1, 100])  # the same B and total_q, other splits
    lens = ([100, 9, 1024, 7, 130], [640, 129, 33, 1000, 8], [1024, 1, 500, 77, 100])
    states = [step_state(geom, T, n, D, seed) for T, n, seed in zip(Ts, lens, (2, 3, 4))]

    def attend(pkg, qd, kp, vp, bd, sl, cd, o, lse):
        pkg.fa2_prefill_paged_varlen_bf16(qd, kp, vp, bd, sl, cd, o, lse)

    def reference(o, lse, s, what):
        ro, rl = vr.ref_prefill_paged_varlen(s["q"], *s["full"], s["lens"], s["cu"])
        seq = slice(s["cu"][0], s["cu"][-1])
        emul = br.emul_prefill_paged_varlen(s["q"], *s["full"], s["lens"], s["cu"])
        at.check(o[seq], lse[seq], ro[seq], rl[seq], emul[seq], "append + prefill D=%d %s lens=%s" % (D, what, s["lens"]))

    captured_step(dev, states, attend, reference)


@pytest.mark.parametrize("D", DS)
def test_graph_replay_of_append_and_multi_decode_for_a_T_1_batch(built, dev, D):
    """A decode step: one new token per sequence, cu_q = arange(B + 1); the attention is the multi entry on q seen as [B,1,Hq,D]."""
    geom = (2, 4, 16, 19)
    B = 5
    lens = ([1, 128, 129, 300, 304], [304, 17, 1, 200, 128], [64, 65, 2, 303, 16])
    states = [step_state(geom, [1] * B, n, D, seed, spare=0) for n, seed in zip(lens, (5, 6, 7))]

    def attend(pkg, qd, kp, vp, bd, sl, cd, o, lse):
        pkg.fa2_decode_paged_multi_bf16(qd[:, None], kp, vp, bd, sl, o[:, None], lse[:, None])

    def reference(o, lse, s, what):
        q4 = s["q"][:, None]
        ro, rl = mr.ref_decode_paged_multi(q4, *s["full"], s["lens"])
        at.check(o[:, None], lse[:, None], ro, rl, br.emul_decode_paged_multi(q4, *s["full"], s["lens"]),
                 "append + multi D=%d %s lens=%s" % (D, what, s["lens"]))

    captured_step(dev, states, attend, reference)
