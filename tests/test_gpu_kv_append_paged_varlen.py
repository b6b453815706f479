"""GPU: the packed variable-length paged KV-cache append (cuda_learn_notes_amd.kv_append_paged_varlen, cln_kv_append_paged_varlen;
csrc/kv_append_paged_varlen.cuh) bit for bit against B fixed-T kv_append_paged calls, one per sequence, on a copy of the same pools, and against
the per-sequence CPU reference of tests/prefill_varlen_reference.py under kv_append_reference.bound. Pools come from
paged_decode_reference.make_pool (NaN poison pages, shuffled placement) and are compared as int16; the packed tensors carry spare rows in front
of cu_q[0] and behind cu_q[B], filled with 6e4 (inputs) and NaN (q_out), which the call must neither read nor write."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_append_reference as kr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import prefill_varlen_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu

DS = [64, 128]
MODE_NAMES = ("none", "half", "interleaved")
CASE_IDS = ["x".join(map(str, g)) for g, _ in vr.CASES]
FIRST, SPARE = 3, 5


def bits(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def problem(ci, D):
    """fp16 packed (k_new, v_new [total_q,Hkv,D], q [total_q,Hq,D]) with 6e4 in the rows outside the sequences, the offsets, and the dense k, v
    [B,Hkv,Nmax,D] the pools are cut from; on the CPU, made once and never modified."""
    (Hkv, G, page, mp), T = vr.CASES[ci]
    g = torch.Generator().manual_seed(31 * ci + D)
    cu = vr.cu_of(T, FIRST)
    tq = cu[-1] + SPARE
    k_new, v_new, q = (torch.randn(tq, H, D, generator=g).half() for H in (Hkv, Hkv, Hkv * G))
    for t in (k_new, v_new, q):
        t[t == 0] = 1.0
        t[:FIRST], t[cu[-1]:] = 6e4, 6e4
    k, v = (torch.randn(len(T), Hkv, page * mp, D, generator=g).half() for _ in range(2))
    return k_new, v_new, q, tuple(cu), k, v


@functools.lru_cache(maxsize=None)
def random_table(max_pos, D):
    """Uniform in [-1, 1], not real sines: a wrong row or column of the table gives a wrong number."""
    return torch.rand(max_pos, D, generator=torch.Generator().manual_seed(max_pos + D)) * 2 - 1


def run(k_new, v_new, kp, vp, bt, lens, cu, q=None, table=None, rope="none", inplace=False, dev="cuda"):
    """The varlen call on copies of everything; returns the pools and q_out on the CPU, after asserting that the inputs kept their bits."""
    import cuda_learn_notes_amd as pkg
    knd, vnd, kd, vd, bd = (t.to(dev) for t in (k_new, v_new, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    qd = qo = td = None
    if q is not None:
        qd = q.to(dev)
        qo = qd if inplace else torch.full_like(qd, float("nan"))
    if table is not None:
        td = table.to(dev)
    pkg.kv_append_paged_varlen(knd, vnd, kd, vd, bd, sl, cd, qd, qo, td, rope)
    torch.cuda.synchronize()
    assert torch.equal(bits(knd.cpu()), bits(k_new)) and torch.equal(bits(vnd.cpu()), bits(v_new))
    assert torch.equal(bd.cpu(), bt) and sl.cpu().tolist() == list(lens) and cd.cpu().tolist() == list(cu)
    if q is not None and not inplace:
        assert torch.equal(bits(qd.cpu()), bits(q))
    return kd.cpu(), vd.cpu(), (qo.cpu() if qo is not None else None)


def run_fixed(k_new, v_new, kp, vp, bt, lens, cu, q=None, table=None, rope="none", dev="cuda"):
    """B fixed-T kv_append_paged calls, one per sequence with T_b >= 1, on a copy of the same pools; q_out assembled in the packed layout, NaN
    in the rows of no sequence."""
    import cuda_learn_notes_amd as pkg
    kd, vd = kp.to(dev), vp.to(dev)
    td = table.to(dev) if table is not None else None
    qo = torch.full_like(q, float("nan")) if q is not None else None
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        if hi == lo:
            continue
        qb = q[lo:hi][None].contiguous().to(dev) if q is not None else None
        ob = torch.full_like(qb, float("nan")) if q is not None else None
        pkg.kv_append_paged(k_new[lo:hi][None].contiguous().to(dev), v_new[lo:hi][None].contiguous().to(dev), kd, vd,
                            bt[b:b + 1].contiguous().to(dev), torch.tensor([lens[b]], dtype=torch.int32, device=dev), qb, ob, td, rope)
        if q is not None:
            qo[lo:hi] = ob[0].cpu()
    torch.cuda.synchronize()
    return kd.cpu(), vd.cpu(), qo


def check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q, table, mode, page, what):
    """V and every K row the call does not write bit for bit (so every other byte of both pools is unchanged); the live K rows and q_out within
    kv_append_reference.bound (mode 0: exact); the q_out rows of tokens that are not live zero; the rows of no sequence keep their NaN fill."""
    rk, rv, k_live, rows, dead = vr.ref_append_varlen(k_new, v_new, kp, vp, bt, lens, cu, q, table, mode)
    assert torch.equal(bits(gv), bits(rv)), what
    keep = ~k_live[:, None, :, None].expand_as(gk)
    assert torch.equal(bits(gk)[keep], bits(rk)[keep]) and torch.equal(bits(gk)[keep], bits(kp)[keep]), what
    worst = 0.0
    for (row, b, pos, k_rot, k_mag, q_rot, q_mag) in rows:
        got = gk[int(bt[b, pos // page]), :, pos % page].double()
        if mode == 0:
            assert torch.equal(got, k_rot), what
        else:
            worst = max(worst, ((got - k_rot).abs() / kr.bound(k_rot, k_mag)).max().item())
            if qo is not None:
                worst = max(worst, ((qo[row].double() - q_rot).abs() / kr.bound(q_rot, q_mag)).max().item())
    if qo is not None:
        nan16 = bits(torch.full((1,), float("nan"), dtype=torch.half)).item()
        assert bool((bits(qo[:cu[0]]) == nan16).all()) and bool((bits(qo[cu[-1]:]) == nan16).all()), what
        assert bool(torch.isfinite(qo[cu[0]:cu[-1]]).all()), what
        for row in dead:
            assert bool((qo[row] == 0).all()), (what, row)
    print("%s: worst error / bound %.4f over %d live and %d dead tokens" % (what, worst, len(rows), len(dead)))
    assert worst <= 1.0, (what, worst)
    return rows, dead


def lengths(geom, T, k=0):
    """One run from position 0, one that crosses a page boundary, one that ends on the last row of the last page, the rest in between."""
    _, _, page, mp = geom
    Nmax = page * mp
    want = [t for t in T]
    want[0] = T[0]                                   # positions 0 .. T_0 - 1
    if len(T) > 1:
        want[-1] = Nmax                              # ends on the last row of the last page
    for b in range(1, len(T) - 1):
        want[b] = min(page * (b + k) - 1 + T[b], Nmax)  # starts on the last row of a page
    return want


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("ci", range(len(vr.CASES)), ids=CASE_IDS)
def test_bits_of_the_fixed_T_calls_and_the_reference(built, dev, ci, mode, D):
    geom, T = vr.CASES[ci]
    page, Nmax = geom[2], geom[2] * geom[3]
    k_new, v_new, q, cu, k, v = problem(ci, D)
    lens = lengths(geom, T)
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=ci)
    table = random_table(Nmax, D) if mode else None
    args = (q, table, MODE_NAMES[mode]) if mode else ()
    gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, cu, *args)
    fk, fv, fq = run_fixed(k_new, v_new, kp, vp, bt, lens, cu, *args)
    assert torch.equal(bits(gk), bits(fk)) and torch.equal(bits(gv), bits(fv)) and not torch.equal(bits(gk), bits(kp))
    if mode:
        assert torch.equal(bits(qo), bits(fq))
    rows, dead = check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q if mode else None, table, mode, page,
                                 "D=%d %s T=%s %s" % (D, geom, T, MODE_NAMES[mode]))
    assert len(rows) == sum(T) and not dead
    if mode == 1:  # K alone: no q rows in the grid
        ak, av, none = run(k_new, v_new, kp, vp, bt, lens, cu, None, table, "half")
        assert none is None and torch.equal(bits(ak), bits(gk)) and torch.equal(bits(av), bits(gv))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tokens_without_a_place_write_nothing(built, dev, mode, D):
    """T = [40, 0, 1, 33, 130] on 1024 rows of cache with a table of 1000 rows: len < T_b (7 of 40 live), a T_b = 0 sequence with a length, len = 0,
    positions at and past max_pos (1000 .. 1009 of the run 977 .. 1009, with a rotation), and a run that passes the capacity (len = 1024 + 30)."""
    ci = 0
    geom, T = vr.CASES[ci]
    page, Nmax = geom[2], geom[2] * geom[3]
    k_new, v_new, q, cu, k, v = problem(ci, D)
    lens = [7, 77, 0, 1010, Nmax + 30]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=2)
    table = random_table(Nmax, D)[:1000].contiguous() if mode else None
    args = (q, table, MODE_NAMES[mode]) if mode else ()
    gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, cu, *args)
    fk, fv, fq = run_fixed(k_new, v_new, kp, vp, bt, lens, cu, *args)
    assert torch.equal(bits(gk), bits(fk)) and torch.equal(bits(gv), bits(fv))
    if mode:
        assert torch.equal(bits(qo), bits(fq))
    rows, dead = check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, q if mode else None, table, mode, page,
                                 "D=%d dead tokens %s" % (D, MODE_NAMES[mode]))
    live4 = 76 if mode else 100  # positions 924 .. 1023 of the run 924 .. 1053, of them 924 .. 999 below max_pos
    live3 = 23 if mode else 33  # 977 .. 999 below max_pos
    assert len(rows) == 7 + live3 + live4 and len(dead) == sum(T) - len(rows)
    assert [r[0] for r in rows][:7] == list(range(cu[0] + 33, cu[0] + 40))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [1, 2])
def test_q_in_place_gives_the_bits_of_the_out_of_place_call(built, dev, mode, D):
    ci = 2
    geom, T = vr.CASES[ci]  # G = 8, T = [16, 17, 0, 2]
    page, Nmax = geom[2], geom[2] * geom[3]
    k_new, v_new, q, cu, k, v = problem(ci, D)
    lens = [10, 100, 50, Nmax + 1]  # dead tokens in front of the first run and behind the last
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=5)
    table = random_table(Nmax, D)
    out = run(k_new, v_new, kp, vp, bt, lens, cu, q, table, MODE_NAMES[mode])
    inp = run(k_new, v_new, kp, vp, bt, lens, cu, q, table, MODE_NAMES[mode], inplace=True)
    assert torch.equal(bits(out[0]), bits(inp[0])) and torch.equal(bits(out[1]), bits(inp[1]))
    lo, hi = cu[0], cu[-1]
    assert torch.equal(bits(out[2][lo:hi]), bits(inp[2][lo:hi])) and not torch.equal(bits(inp[2][lo:hi]), bits(q[lo:hi]))
    assert torch.equal(bits(inp[2][:lo]), bits(q[:lo])) and torch.equal(bits(inp[2][hi:]), bits(q[hi:]))  # in place: the spare rows keep q's 6e4


def test_python_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    f = pkg.kv_append_paged_varlen
    B, tq, Hkv, Hq, page, mp, D, P = 2, 7, 2, 8, 16, 4, 64, 9
    h = lambda *s: torch.zeros(*s, dtype=torch.half, device=dev)  # noqa: E731
    kn, vn, kp, vp, q, qo = h(tq, Hkv, D), h(tq, Hkv, D), h(P, Hkv, page, D), h(P, Hkv, page, D), h(tq, Hq, D), h(tq, Hq, D)
    bt = torch.zeros(B, mp, dtype=torch.int32, device=dev)
    sl = torch.zeros(B, dtype=torch.int32, device=dev)  # every token at a negative position: a call that gets through writes nothing
    cu = torch.tensor([0, 3, 7], dtype=torch.int32, device=dev)
    tab = torch.zeros(64, D, device=dev)
    f(kn, vn, kp, vp, bt, sl, cu)
    f(kn, vn, kp, vp, bt, sl, cu, q, qo, tab, "half")
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: headdim 96 not supported"):
        f(h(tq, Hkv, 96), h(tq, Hkv, 96), h(P, Hkv, page, 96), h(P, Hkv, page, 96), bt, sl, cu)
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: page size 48 not supported"):
        f(kn, vn, h(P, Hkv, 48, D), h(P, Hkv, 48, D), bt, sl, cu)
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: rope 'neox' not supported"):
        f(kn, vn, kp, vp, bt, sl, cu, q, qo, tab, "neox")
    with pytest.raises(RuntimeError, match="no multiple"):
        f(kn, vn, kp, vp, bt, sl, cu, h(tq, 3, D), h(tq, 3, D), tab, "half")
    with pytest.raises(RuntimeError, match="status -1"):
        f(kn, vn, kp, kp, bt, sl, cu)  # the pools are one tensor
    bad = [
        lambda: f(kn.float(), vn, kp, vp, bt, sl, cu),                                   # dtype
        lambda: f(kn, vn, kp, vp, bt, sl, cu.long()),
        lambda: f(kn, vn, kp, vp, bt, sl, cu, q, qo, tab.half(), "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, cu.cpu()),                                     # device
        lambda: f(kn, vn, kp, vp, bt.cpu(), sl, cu),
        lambda: f(kn, vn, kp, vp, bt, sl, cu[:2].contiguous()),                          # shape: a cu_q of length B
        lambda: f(kn[None], vn, kp, vp, bt, sl, cu),
        lambda: f(kn, vn[:5].contiguous(), kp, vp, bt, sl, cu),
        lambda: f(kn, vn, kp, vp, bt, sl[:1], cu),
        lambda: f(kn, vn, kp, vp, bt, sl, cu, q, qo[:, :4].contiguous(), tab, "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, cu, q, qo, None, "half"),                      # the pointer rules of rope
        lambda: f(kn, vn, kp, vp, bt, sl, cu, q, None, tab, "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, cu, q, qo, tab),
    ]
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
    torch.cuda.synchronize()
    assert bool((kp == 0).all()) and bool((vp == 0).all()) and bool((qo == 0).all())
