"""GPU: the paged KV-cache append with the rotary embedding fused in (cuda_learn_notes_amd.kv_append_paged, cln_kv_append_paged;
csrc/kv_append_paged.cuh) against the CPU reference of tests/kv_append_reference.py. Every case runs on a pool of
paged_decode_reference.make_pool: more pages than needed, the live pages placed by a seeded permutation with the sequences interleaved, every
page no live entry names filled with NaN, every table entry past the length pointing at an in-range poison page of NaN -- a kernel that follows a
wrong entry or writes a row too many changes a byte the comparison sees, it does not fault. Pools are compared as int16 (they hold NaN). Rotated
values are held to kv_append_reference.bound, which is derived from the number formats; every such case prints its worst error / bound ratio
before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import kv_append_reference as kr  # noqa: E402
import multi_decode_reference as mr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu

B = 3
DS = [64, 128]
HEADS = [(1, 1), (3, 6), (2, 16)]  # (Hkv, Hq); 3 KV heads: an index that shifts where it should multiply goes wrong
PAGES = [16, 256]
TS = [1, 2, 8, 19]  # 19 tokens from row 15 on span three 16-row pages
MODE_NAMES = ("none", "half", "interleaved")
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def max_pages_of(page):
    return 3 if page == 16 else 2


def lengths(page, T):
    """One sequence starts at position 0, one run crosses the first page boundary mid-run (T = 1: it starts the second page), one ends on the last
    row of the last page."""
    return [T, (page - 1 if T > 1 else page) + T, max_pages_of(page) * page]


def nonzero_half(*shape, g):
    x = torch.randn(*shape, generator=g).half()
    x[x == 0] = 1.0  # no zeros: the exact-rotation cases compare values with ==, and a signed zero would pass for the other one
    return x


@functools.lru_cache(maxsize=None)
def problem(D, heads, page, T):
    """fp16 (k_new, v_new [B,T,Hkv,D], q [B,T,Hq,D], dense k, v [B,Hkv,Nmax,D] the pools are cut from) on the CPU, made once and never modified."""
    Hkv, Hq = heads
    g = torch.Generator().manual_seed(D + 7 * Hkv + 13 * Hq + page + 31 * T)
    k_new, v_new, q = (nonzero_half(B, T, H, D, g=g) for H in (Hkv, Hkv, Hq))
    k, v = (torch.randn(B, Hkv, max_pages_of(page) * page, D, generator=g).half() for _ in range(2))
    return k_new, v_new, q, k, v


@functools.lru_cache(maxsize=None)
def random_table(max_pos, D):
    """Uniform in [-1, 1], not real sines: a wrong row or column of the table gives a wrong number."""
    return torch.rand(max_pos, D, generator=torch.Generator().manual_seed(max_pos + D)) * 2 - 1


def bits(t):
    return t.view(torch.int16)


def run(k_new, v_new, kp, vp, bt, lens, q=None, table=None, rope="none", inplace=False, dev="cuda"):
    """The call on copies of everything; returns the pools and q_out on the CPU, after asserting that the inputs kept their bits."""
    import cuda_learn_notes_amd as pkg
    knd, vnd, kd, vd, bd = (t.to(dev) for t in (k_new, v_new, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    qd = qo = td = None
    if q is not None:
        qd = q.to(dev)
        qo = qd if inplace else torch.full_like(qd, float("nan"))
    if table is not None:
        td = table.to(dev)
    pkg.kv_append_paged(knd, vnd, kd, vd, bd, sl, qd, qo, td, rope)
    torch.cuda.synchronize()
    assert torch.equal(bits(knd.cpu()), bits(k_new)) and torch.equal(bits(vnd.cpu()), bits(v_new))
    assert torch.equal(bd.cpu(), bt) and sl.cpu().tolist() == list(lens)
    if q is not None and not inplace:
        assert torch.equal(bits(qd.cpu()), bits(q))
    if table is not None:
        assert torch.equal(td.cpu(), table)
    return kd.cpu(), vd.cpu(), (qo.cpu() if qo is not None else None)


def check_rotated(kp, vp, qo, ref, bt, lens, T, page, what):
    """V and every K row the call does not write bit for bit; every element of the live K rows and of q_out within the derived bound; the q_out
    rows of tokens that are not live zero. Returns the worst error / bound."""
    assert torch.equal(bits(vp), bits(ref.v_pages)), what
    keep = ~ref.k_live[:, None, :, None].expand_as(kp)
    assert torch.equal(bits(kp)[keep], bits(ref.k_pages)[keep]), what
    worst = 0.0
    for (b, t) in ref.live:
        pos = int(lens[b]) - T + t
        got = kp[int(bt[b, pos // page]), :, pos % page].double()
        ratio = ((got - ref.k_rot[b, t]).abs() / kr.bound(ref.k_rot[b, t], ref.k_mag[b, t])).max().item()
        worst = max(worst, ratio)
    if qo is not None:
        assert bool(torch.isfinite(qo).all()), what
        worst = max(worst, ((qo.double() - ref.q_rot).abs() / kr.bound(ref.q_rot, ref.q_mag)).max().item())
        dead = torch.ones(qo.shape[:2], dtype=torch.bool)
        for (b, t) in ref.live:
            dead[b, t] = False
        assert bool((qo[dead] == 0).all()), what
    print("%s: worst error / bound %.4f over %d live tokens" % (what, worst, len(ref.live)))
    assert worst <= 1.0, (what, worst)
    return worst


GRID = [(D, heads, page, T) for D in DS for heads in HEADS for page in PAGES for T in TS]
grid_ids = ["D%d-H%s-p%d-T%d" % (D, ids(h), p, T) for (D, h, p, T) in GRID]


@pytest.mark.parametrize("D,heads,page,T", GRID, ids=grid_ids)
def test_no_rope_is_an_exact_scatter(built, dev, D, heads, page, T):
    k_new, v_new, q, k, v = problem(D, heads, page, T)
    lens = lengths(page, T)
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=T)
    ref = kr.ref_append(k_new, v_new, kp, vp, bt, lens, None, None, 0)
    assert len(ref.live) == B * T
    gk, gv, _ = run(k_new, v_new, kp, vp, bt, lens)
    assert torch.equal(bits(gk), bits(ref.k_pages)) and torch.equal(bits(gv), bits(ref.v_pages))
    assert not torch.equal(bits(gk), bits(kp))


@pytest.mark.parametrize("D,heads,page,T", GRID, ids=grid_ids)
def test_unit_tables_rotate_exactly(built, dev, D, heads, page, T):
    """cos = 1, sin = 0: the pools of the call without a rotation, and q_out = q. cos = 0, sin = 1: every pair becomes (-x2, x1) exactly."""
    k_new, v_new, q, k, v = problem(D, heads, page, T)
    lens = lengths(page, T)
    cap = max_pages_of(page) * page
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=T)
    plain = kr.ref_append(k_new, v_new, kp, vp, bt, lens, None, None, 0)
    one, zero = torch.ones(cap, D // 2), torch.zeros(cap, D // 2)
    for mode in (1, 2):
        gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, q, torch.cat((one, zero), dim=1), MODE_NAMES[mode])
        assert torch.equal(bits(gk), bits(plain.k_pages)) and torch.equal(bits(gv), bits(plain.v_pages)), mode
        assert bool((qo == q).all()), mode
        table = torch.cat((zero, one), dim=1)
        ref = kr.ref_append(k_new, v_new, kp, vp, bt, lens, q, table, mode)  # (-x2, x1) in float64: exact, and exact again in fp16
        gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, q, table, MODE_NAMES[mode])
        assert torch.equal(bits(gv), bits(plain.v_pages)), mode
        keep = ~ref.k_live[:, None, :, None].expand_as(gk)
        assert torch.equal(bits(gk)[keep], bits(kp)[keep]), mode
        live = ~keep
        assert bool((gk[live] == ref.k_pages[live]).all()) and bool((qo.double() == ref.q_rot).all()), mode
        x = q[0, 0, 0]
        want = torch.cat((-x[D // 2:], x[:D // 2])) if mode == 1 else torch.stack((-x[1::2], x[0::2]), dim=-1).flatten()
        assert bool((qo[0, 0, 0] == want).all()), mode  # the reference's pairing, spelled out once more


@pytest.mark.parametrize("D,heads,page,T", GRID, ids=grid_ids)
def test_general_rotation_within_the_derived_bound(built, dev, D, heads, page, T):
    k_new, v_new, q, k, v = problem(D, heads, page, T)
    lens = lengths(page, T)
    table = random_table(max_pages_of(page) * page, D)
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=T + 1)
    for mode in (1, 2):
        ref = kr.ref_append(k_new, v_new, kp, vp, bt, lens, q, table, mode)
        assert len(ref.live) == B * T
        gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, q, table, MODE_NAMES[mode])
        check_rotated(gk, gv, qo, ref, bt, lens, T, page, "D=%d H=%s page=%d T=%d %s" % (D, heads, page, T, MODE_NAMES[mode]))
        if mode == 1 and T == 8:  # K alone: no q rows in the grid
            ak, av, none = run(k_new, v_new, kp, vp, bt, lens, None, table, "half")
            assert none is None and torch.equal(bits(ak), bits(gk)) and torch.equal(bits(av), bits(gv))


# lengths that leave tokens without a place, (Hkv, Hq) = (3, 6), page 16, three pages (48 rows)
DEAD = {
    "short": lambda T: [3, 0, -7],                       # len < T: only the last 3 tokens are live; len = 0 and len < 0: none is
    "long": lambda T: [48 + 2, 2 ** 31 - 1, -2 ** 31],   # len > capacity: the last 2 tokens are not live; the int32 extremes: none is, no overflow
    "mixed": lambda T: [48 + 4, 5, 48 + T],              # the last 4 not live; the last 5 live; the first token one past the last row
}


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("case", sorted(DEAD))
@pytest.mark.parametrize("T", [5, 19])
def test_tokens_without_a_place_write_nothing(built, dev, D, case, T):
    heads, page = (3, 6), 16
    k_new, v_new, q, k, v = problem(D, heads, page, T)
    lens = DEAD[case](T)
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=2)
    ref0 = kr.ref_append(k_new, v_new, kp, vp, bt, lens, None, None, 0)
    want_live = {"short": [(0, t) for t in range(T - 3, T)], "long": [(0, t) for t in range(T - 2)],
                 "mixed": [(0, t) for t in range(T - 4)] + ([(1, t) for t in range(T)] if T == 5 else [(1, t) for t in range(T - 5, T)])}[case]
    assert ref0.live == want_live
    gk, gv, _ = run(k_new, v_new, kp, vp, bt, lens)
    assert torch.equal(bits(gk), bits(ref0.k_pages)) and torch.equal(bits(gv), bits(ref0.v_pages))
    table = random_table(48, D)
    for mode in (1, 2):
        ref = kr.ref_append(k_new, v_new, kp, vp, bt, lens, q, table, mode)
        assert ref.live == want_live
        gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, q, table, MODE_NAMES[mode])
        check_rotated(gk, gv, qo, ref, bt, lens, T, page, "D=%d T=%d %s %s" % (D, T, case, MODE_NAMES[mode]))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [1, 2])
def test_positions_at_or_past_max_pos_are_not_live(built, dev, D, mode):
    """A table shorter than the capacity: 48 rows of cache, 40 table rows. Of the run at positions 37 .. 41 the last two tokens write nothing and
    get zero q_out rows; the sequence that ends on row 47 writes nothing at all."""
    heads, page, T = (3, 6), 16, 5
    k_new, v_new, q, k, v = problem(D, heads, page, T)
    lens = [42, 5, 48]
    table = random_table(48, D)[:40].contiguous()
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=4)
    ref = kr.ref_append(k_new, v_new, kp, vp, bt, lens, q, table, mode)
    assert ref.live == [(0, 0), (0, 1), (0, 2)] + [(1, t) for t in range(T)]
    gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, q, table, MODE_NAMES[mode])
    check_rotated(gk, gv, qo, ref, bt, lens, T, page, "D=%d max_pos=40 %s" % (D, MODE_NAMES[mode]))
    assert bool((qo[0, 3:] == 0).all()) and bool((qo[2] == 0).all()) and bool((qo[0, :3] != 0).any())


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("lens", [[19, 34, 48], [3, 48 + 2, 0]], ids=ids)
def test_q_in_place_gives_the_bits_of_the_out_of_place_call(built, dev, D, mode, lens):
    heads, page, T = (2, 16), 16, 19
    k_new, v_new, q, k, v = problem(D, heads, page, T)
    table = random_table(48, D)
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=5)
    out = run(k_new, v_new, kp, vp, bt, lens, q, table, MODE_NAMES[mode])
    inp = run(k_new, v_new, kp, vp, bt, lens, q, table, MODE_NAMES[mode], inplace=True)
    for a, b in zip(out, inp):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(bits(inp[2]), bits(q))


def step_problem(D, T, page, mp, lens, seed):
    """A decode step: dense fp16 k, v [B,Hkv,Nmax,D] and q [B,T,Hq,D] with Hkv = 2, G = 4; the T newest rows of every sequence as k_new, v_new;
    and `hole`, the mask [B,Nmax] of those rows."""
    Hkv, Hq = 2, 8
    g = torch.Generator().manual_seed(seed + D + T)
    k, v = (torch.randn(B, Hkv, mp * page, D, generator=g).half() for _ in range(2))
    q = torch.randn(B, T, Hq, D, generator=g).half()
    hole = torch.zeros(B, mp * page, dtype=torch.bool)
    k_new, v_new = torch.zeros(B, T, Hkv, D).half(), torch.zeros(B, T, Hkv, D).half()
    for b in range(B):
        assert T <= lens[b] <= mp * page
        hole[b, lens[b] - T:lens[b]] = True
        k_new[b], v_new[b] = k[b, :, lens[b] - T:lens[b]].transpose(0, 1), v[b, :, lens[b] - T:lens[b]].transpose(0, 1)
    return k, v, q, k_new, v_new, hole


def with_holes(x, hole):
    """The dense cache before the step: the rows the step will write hold NaN."""
    y = x.clone()
    y.transpose(1, 2)[hole] = float("nan")
    return y


def attend(q, kp, vp, bt, sl, ws=None):
    import cuda_learn_notes_amd as pkg
    o = torch.full_like(q, float("nan"))
    lse = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device=q.device)
    pkg.fa2_decode_paged_multi(q, kp, vp, bt, sl, o, lse, ws)
    return o, lse


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("T", [1, 5])
def test_append_then_attention_equals_attention_on_a_cpu_built_pool(built, dev, D, T):
    import cuda_learn_notes_amd as pkg
    page, mp = 16, 4
    lens = [T, 17 + T // 2, 64]
    k, v, q, k_new, v_new, hole = step_problem(D, T, page, mp, lens, seed=1)
    full = pr.make_pool(k, v, page, lens, seed=6)
    before = pr.make_pool(with_holes(k, hole), with_holes(v, hole), page, lens, seed=6)
    assert torch.equal(full[2], before[2]) and not torch.equal(bits(full[0]), bits(before[0]))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    qd, bd = q.to(dev), full[2].to(dev)
    kd, vd = before[0].to(dev), before[1].to(dev)
    pkg.kv_append_paged(k_new.to(dev), v_new.to(dev), kd, vd, bd, sl)
    o, lse = attend(qd, kd, vd, bd, sl)
    o2, lse2 = attend(qd, full[0].to(dev), full[1].to(dev), bd, sl)
    torch.cuda.synchronize()
    assert torch.equal(bits(kd.cpu()), bits(full[0])) and torch.equal(bits(vd.cpu()), bits(full[1]))
    assert bool(torch.isfinite(o).all()) and torch.equal(o, o2) and torch.equal(lse, lse2)


def rotated_step(D, T, page, mp, lens, seed):
    """step_problem with the NeoX rotation by a real table: the cache holds rotated K rows. Returns the unrotated new rows and q for the call, the
    pools before the step, and for the reference the full rotated pools and the rotated q, both fp64-rotated and rounded once to fp16."""
    import cuda_learn_notes_amd as pkg
    k, v, q, k_new, v_new, hole = step_problem(D, T, page, mp, lens, seed)
    table = pkg.kv_append_rope_table(mp * page, D)
    k_rot = torch.stack([kr.rotate(k[:, :, p], table[p], 1)[0] for p in range(mp * page)], dim=2).half()
    q_rot = torch.stack([torch.stack([kr.rotate(q[b, t], table[lens[b] - T + t], 1)[0] for t in range(T)]) for b in range(B)]).half()
    full = pr.make_pool(k_rot, v, page, lens, seed=7)
    before = pr.make_pool(with_holes(k_rot, hole), with_holes(v, hole), page, lens, seed=7)
    assert torch.equal(full[2], before[2])
    return q, k_new, v_new, table, before, full, q_rot


def check_attention(o, lse, q_rot, full, lens, what):
    ro, rl = mr.ref_decode_paged_multi(q_rot, full[0], full[1], full[2], lens)
    eo, el = (o.double() - ro).abs().max().item(), (lse.double() - rl).abs().max().item()
    print("%s: O err %.3e / bound %.3e   LSE err %.3e / bound %.3e" % (what, eo, dr.fa_tol(ro), el, dr.lse_tol(rl)))
    assert bool(torch.isfinite(o).all()) and eo <= dr.fa_tol(ro) and el <= dr.lse_tol(rl), (what, eo, el)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("T", [1, 5])
def test_rotate_append_attend_against_the_fp64_reference(built, dev, D, T):
    import cuda_learn_notes_amd as pkg
    page, mp = 16, 4
    lens = [T, 17 + T // 2, 64]
    q, k_new, v_new, table, before, full, q_rot = rotated_step(D, T, page, mp, lens, seed=2)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    kd, vd, bd = (t.to(dev) for t in before)
    qo = torch.full(q.shape, float("nan"), dtype=torch.half, device=dev)
    pkg.kv_append_paged(k_new.to(dev), v_new.to(dev), kd, vd, bd, sl, q.to(dev), qo, table.to(dev), "half")
    o, lse = attend(qo, kd, vd, bd, sl)
    torch.cuda.synchronize()
    assert torch.equal(bits(vd.cpu()), bits(full[1]))
    check_attention(o.cpu(), lse.cpu(), q_rot, full, lens, "D=%d T=%d rope half" % (D, T))


@pytest.mark.parametrize("D", DS)
def test_graph_replay_of_the_step_reads_everything_from_the_device(built, dev, D):
    """Append, attention and the merge of its splits captured as one line of kernels on one stream; lengths, table, pools, new rows and q changed in
    place; the replay equals the eager step on the same device state bit for bit, and the reference."""
    import cuda_learn_notes_amd as pkg
    page, mp, T = 16, 32, 5
    S, C, need = pkg.fa2_decode_paged_multi_plan(B, T, 8, 2, mp, page, D)
    assert S > 1
    lens1, lens2 = [100, 512, 7], [110, 5, 512]  # 40 live pages both: pools of one shape
    first, second = rotated_step(D, T, page, mp, lens1, seed=3), rotated_step(D, T, page, mp, lens2, seed=4)
    assert first[4][0].shape == second[4][0].shape and not torch.equal(first[4][2], second[4][2])
    q, k_new, v_new, table, before, full, q_rot = first
    qd, knd, vnd, td = (t.to(dev) for t in (q, k_new, v_new, table))
    kd, vd, bd = (t.to(dev) for t in before)
    sl = torch.tensor(lens1, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    qo, og = torch.zeros_like(qd), torch.zeros_like(qd)
    lg = torch.zeros(B, T, 8, dtype=torch.float32, device=dev)

    def step(kp, vp, q_out, o, lse):
        pkg.kv_append_paged(knd, vnd, kp, vp, bd, sl, qd, q_out, td, "half")
        pkg.fa2_decode_paged_multi(q_out, kp, vp, bd, sl, o, lse, ws)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(kd, vd, qo, og, lg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(kd, vd, qo, og, lg)
    q, k_new, v_new, table, before, full, q_rot = second
    sl.copy_(torch.tensor(lens2, dtype=torch.int32))
    qd.copy_(q), knd.copy_(k_new), vnd.copy_(v_new), kd.copy_(before[0]), vd.copy_(before[1]), bd.copy_(before[2])
    qo.zero_(), og.zero_(), lg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    ke, ve = before[0].to(dev), before[1].to(dev)
    qe, oe, le = torch.empty_like(qd), torch.empty_like(qd), torch.empty_like(lg)
    step(ke, ve, qe, oe, le)
    torch.cuda.synchronize()
    assert torch.equal(bits(kd), bits(ke)) and torch.equal(bits(vd), bits(ve)) and torch.equal(qo, qe) and torch.equal(og, oe) and torch.equal(lg, le)
    assert torch.equal(bits(vd.cpu()), bits(full[1]))
    check_attention(og.cpu(), lg.cpu(), q_rot, full, lens2, "graph replay D=%d" % D)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_two_calls_on_equal_inputs_give_equal_bits(built, dev, D, mode):
    heads, page, T = (3, 6), 16, 19
    k_new, v_new, q, k, v = problem(D, heads, page, T)
    lens = [19, 34, 48 + 3]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=8)
    args = (q, random_table(48, D), MODE_NAMES[mode]) if mode else ()
    a, b = run(k_new, v_new, kp, vp, bt, lens, *args), run(k_new, v_new, kp, vp, bt, lens, *args)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    assert mode == 0 or torch.equal(bits(a[2]), bits(b[2]))


def test_python_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    f = pkg.kv_append_paged
    Bq, T, Hkv, Hq, page, mp, D, P = 2, 3, 2, 8, 16, 4, 64, 9
    h = lambda *s: torch.zeros(*s, dtype=torch.half, device=dev)  # noqa: E731
    kn, vn, kp, vp, q, qo = h(Bq, T, Hkv, D), h(Bq, T, Hkv, D), h(P, Hkv, page, D), h(P, Hkv, page, D), h(Bq, T, Hq, D), h(Bq, T, Hq, D)
    bt = torch.zeros(Bq, mp, dtype=torch.int32, device=dev)
    sl = torch.zeros(Bq, dtype=torch.int32, device=dev)  # every token at a negative position: a call that gets through writes nothing
    tab = torch.zeros(64, D, device=dev)
    f(kn, vn, kp, vp, bt, sl)
    f(kn, vn, kp, vp, bt, sl, q, qo, tab, "half")
    with pytest.raises(RuntimeError, match="kv_append_paged: headdim 96 not supported"):
        f(h(Bq, T, Hkv, 96), h(Bq, T, Hkv, 96), h(P, Hkv, page, 96), h(P, Hkv, page, 96), bt, sl)
    with pytest.raises(RuntimeError, match="kv_append_paged: page size 48 not supported"):
        f(kn, vn, h(P, Hkv, 48, D), h(P, Hkv, 48, D), bt, sl)
    with pytest.raises(RuntimeError, match="kv_append_paged: rope 'neox' not supported"):
        f(kn, vn, kp, vp, bt, sl, q, qo, tab, "neox")
    with pytest.raises(RuntimeError, match="no multiple"):
        f(kn, vn, kp, vp, bt, sl, h(Bq, T, 3, D), h(Bq, T, 3, D), tab, "half")
    with pytest.raises(RuntimeError, match="status -1"):
        f(kn, vn, kp, kp, bt, sl)  # the pools are one tensor
    bad = [
        lambda: f(kn.float(), vn, kp, vp, bt, sl),                                   # dtype
        lambda: f(kn, vn, kp, vp.float(), bt, sl),
        lambda: f(kn, vn, kp, vp, bt.long(), sl),
        lambda: f(kn, vn, kp, vp, bt, sl.long()),
        lambda: f(kn, vn, kp, vp, bt, sl, q, qo, tab.half(), "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, q.float(), qo, tab, "half"),
        lambda: f(kn.cpu(), vn, kp, vp, bt, sl),                                     # device
        lambda: f(kn, vn, kp, vp, bt.cpu(), sl),
        lambda: f(kn, vn, kp, vp, bt, sl.cpu()),
        lambda: f(kn, vn, kp, vp, bt, sl, q, qo, tab.cpu(), "half"),
        lambda: f(kn[:, 0].contiguous(), vn, kp, vp, bt, sl),                        # shape
        lambda: f(kn, vn[:, :2].contiguous(), kp, vp, bt, sl),
        lambda: f(kn, vn, kp, vp[:4].contiguous(), bt, sl),
        lambda: f(kn, vn, kp, vp, bt[:1].contiguous(), sl),
        lambda: f(kn, vn, kp, vp, bt, sl[:1]),
        lambda: f(kn, vn, kp, vp, bt, sl, q, qo[:, :, :4].contiguous(), tab, "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, q, qo, tab[:, :32].contiguous(), "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, q, qo, tab.view(-1), "half"),
        lambda: f(kn.transpose(1, 2).contiguous().transpose(1, 2), vn, kp, vp, bt, sl),   # not contiguous
        lambda: f(kn, vn, kp.transpose(1, 2).contiguous().transpose(1, 2), vp, bt, sl),
        lambda: f(kn, vn, kp, vp, bt.t().contiguous().t(), sl),
        lambda: f(kn, vn, kp, vp, bt, sl, q, qo, tab.t().contiguous().t(), "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, q, qo, None, "half"),                      # the pointer rules of rope
        lambda: f(kn, vn, kp, vp, bt, sl, q, None, tab, "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, None, qo, tab, "interleaved"),
        lambda: f(kn, vn, kp, vp, bt, sl, q, qo, tab),
        lambda: f(kn, vn, kp, vp, bt, sl, rope_table=tab),
    ]
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
    torch.cuda.synchronize()
    assert bool((kp == 0).all()) and bool((vp == 0).all()) and bool((qo == 0).all())
