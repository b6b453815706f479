"""GPU: the quantising append into an FP8 paged KV cache (cuda_learn_notes_amd.kv_append_paged_fp8, cln_kv_append_paged_fp8;
csrc/kv_append_paged_fp8.cuh) against the CPU reference of tests/fp8_kv_reference.py. Every pool is pre-filled with a sentinel byte and stands
between two guard bands of another byte inside one allocation, the live pages are placed by a seeded permutation with the sequences interleaved
and every table entry past the length points at an in-range page: a kernel that follows a wrong entry or writes a row too many changes a byte
the comparison sees, it does not fault. Pools are compared as bytes. Rotated rows are held to fp8_kv_reference.bound, which is derived from the
number formats; such a case prints its worst error / bound before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import kv_append_reference as kr  # noqa: E402

pytestmark = pytest.mark.gpu

B = 3
DS = [64, 128]
HEADS = [(1, 1), (1, 4), (5, 5), (5, 20)]  # (Hkv, Hq): Hq / Hkv in {1, 4}; 5 KV heads: an index that shifts where it should multiply goes wrong
PAGES = [16, 256]
TS = [1, 3, 17]  # 17 tokens from row 15 on span three 16-row pages
MODE_NAMES = ("none", "half", "interleaved")
SENTINEL, GUARD, GB = 0x5A, 0xC3, 4096
ids = lambda s: "x".join(map(str, s))  # noqa: E731
bits = f8.bits


def max_pages_of(page):
    return 3 if page == 16 else 2


def lengths(page, T):
    """One sequence starts at position 0, one run crosses the first page boundary mid-run (T = 1: it starts the second page), one ends on the last
    row of the last page."""
    return [T, (page - 1 if T > 1 else page) + T, max_pages_of(page) * page]


def pow2_scales(Hkv, shift=0):
    """2^(h - 2 + shift): distinct per head, so that a head-index mix-up shows, and exact in every operation of the quantiser."""
    return torch.tensor([2.0 ** (h - 2 + shift) for h in range(Hkv)])


def odd_scales(Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(Hkv, generator=g) * 0.09 + 0.003) * torch.tensor([1.0, 7.0, 0.31, 19.0, 2.3])[:Hkv]


@functools.lru_cache(maxsize=None)
def problem(D, heads, T):
    """fp16 (k_new, v_new [B,T,Hkv,D], q [B,T,Hq,D]) on the CPU, made once and never modified. The new rows are Gaussian in units of 2^(h - 2) 16,
    so a few per cent of them lie beyond 448 scale (the clamp), and some elements are set to the e4m3 subnormal range, to ties, and to +-0."""
    Hkv, Hq = heads
    g = torch.Generator().manual_seed(D + 7 * Hkv + 13 * Hq + 31 * T)
    unit = pow2_scales(Hkv).view(1, 1, Hkv, 1)
    k_new, v_new = ((torch.randn(B, T, Hkv, D, generator=g) * 200 * unit).half() for _ in range(2))
    q = torch.randn(B, T, Hq, D, generator=g).half()
    for x in (k_new, v_new):
        x[..., 0] = 0.0
        x[..., 1] = -0.0
        x[..., 2:6] = (torch.tensor([1.0, 0.5, 1.5, -2.5]) * 2.0 ** -9 * unit).half()   # subnormal codes and their ties
        x[..., 6:10] = (torch.tensor([17.0, -19.0, 449.0, -1e4]) * unit).half()          # ties in the normal range, just past and far past the clamp
        x[..., 10] = (5e-5 * unit[..., 0]).half()                                        # rounds to zero
    return k_new, v_new, q


@functools.lru_cache(maxsize=None)
def random_table(max_pos, D):
    """Uniform in [-1, 1], not real sines: a wrong row or column of the table gives a wrong number."""
    return torch.rand(max_pos, D, generator=torch.Generator().manual_seed(max_pos + D)) * 2 - 1


def sentinel_pool(Hkv, page, D, lens, seed):
    """(k_pages, v_pages, block_table) on the CPU: pools of the sentinel byte, P = 3 live // 2 + 2 pages, the live pages interleaved and placed
    by a seeded permutation, dead table entries pointing at the last page (fp8_kv_reference.make_pool on sentinel caches)."""
    Nmax = max_pages_of(page) * page
    dense = torch.full((B, Hkv, Nmax, D), SENTINEL, dtype=torch.uint8).view(f8.F8)
    kp, vp, bt = f8.make_pool(dense, dense, page, lens, seed=seed)
    bits(kp).fill_(SENTINEL), bits(vp).fill_(SENTINEL)
    return kp, vp, bt


def run(k_new, v_new, kp, vp, bt, lens, ks, vs, q=None, table=None, rope="none", inplace=False, dev="cuda"):
    """The call on copies of everything, the pools inside guard bands; returns the pools and q_out on the CPU, after asserting that the guard
    bands and the inputs kept their bytes."""
    import cuda_learn_notes_amd as pkg
    n = kp.numel()
    bufs = [torch.full((n + 2 * GB,), GUARD, dtype=torch.uint8, device=dev) for _ in range(2)]
    pools = []
    for buf, src in zip(bufs, (kp, vp)):
        buf[GB:GB + n] = bits(src).flatten().to(dev)
        pools.append(buf[GB:GB + n].view(kp.shape).view(f8.F8))
    knd, vnd, bd, ksd, vsd = (t.to(dev) for t in (k_new, v_new, bt, ks, vs))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    qd = qo = td = None
    if q is not None:
        qd = q.to(dev)
        qo = qd if inplace else torch.full_like(qd, float("nan"))
    if table is not None:
        td = table.to(dev)
    pkg.kv_append_paged_fp8(knd, vnd, pools[0], pools[1], bd, sl, ksd, vsd, qd, qo, td, rope)
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf[:GB] == GUARD).all()) and bool((buf[GB + n:] == GUARD).all())
    assert torch.equal(knd.cpu().view(torch.int16), k_new.view(torch.int16)) and torch.equal(vnd.cpu().view(torch.int16), v_new.view(torch.int16))
    assert torch.equal(bd.cpu(), bt) and sl.cpu().tolist() == list(lens) and torch.equal(ksd.cpu(), ks) and torch.equal(vsd.cpu(), vs)
    if q is not None and not inplace:
        assert torch.equal(qd.cpu().view(torch.int16), q.view(torch.int16))
    return pools[0].cpu(), pools[1].cpu(), (qo.cpu() if qo is not None else None)


def report_mismatch(got, want, k_new, what):
    """For the summary, should the hardware's conversion disagree with round-to-nearest-even: the first differing bytes."""
    bad = (bits(got) != bits(want)).nonzero()
    for idx in bad[:8].tolist():
        print("%s: byte %s got 0x%02x want 0x%02x" % (what, idx, int(bits(got)[tuple(idx)]), int(bits(want)[tuple(idx)])))
    return len(bad)


GRID = [(D, heads, page, T) for D in DS for heads in HEADS for page in PAGES for T in TS]
grid_ids = ["D%d-H%s-p%d-T%d" % (D, ids(h), p, T) for (D, h, p, T) in GRID]


@pytest.mark.parametrize("D,heads,page,T", GRID, ids=grid_ids)
def test_exact_bytes_with_power_of_two_scales(built, dev, D, heads, page, T):
    """rope "none": the pool bytes are quantize(...) whatever way the kernel divides, and every other byte keeps the sentinel."""
    k_new, v_new, _ = problem(D, heads, T)
    lens = lengths(page, T)
    ks, vs = pow2_scales(heads[0]), pow2_scales(heads[0], shift=1)
    kp, vp, bt = sentinel_pool(heads[0], page, D, lens, seed=T)
    ref = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, lens, ks, vs, None, None, 0)
    assert len(ref.live) == B * T
    codes = set(bits(ref.k_pages)[ref.k_live[:, None, :, None].expand_as(kp)].tolist())
    assert {0x00, 0x80, 0x7E, 0xFE, 0x01, 0x02} <= codes and 0x7F not in codes and 0xFF not in codes  # zeros, the clamp, subnormals; never NaN
    gk, gv, _ = run(k_new, v_new, kp, vp, bt, lens, ks, vs)
    assert report_mismatch(gk, ref.k_pages, k_new, "K") == 0 and report_mismatch(gv, ref.v_pages, v_new, "V") == 0
    assert not torch.equal(bits(gk), bits(kp))
    written = ref.k_live[:, None, :, None].expand_as(kp)
    assert bool((bits(gk)[~written] == SENTINEL).all()) and bool((bits(gv)[~written] == SENTINEL).all())


@pytest.mark.parametrize("D,heads,page,T", GRID, ids=grid_ids)
def test_exact_bytes_with_arbitrary_scales(built, dev, D, heads, page, T):
    """rope "none", scales that are no power of two: x * (1.0f / scale) in IEEE fp32, clamped, rounded to nearest even, byte for byte."""
    k_new, v_new, _ = problem(D, heads, T)
    lens = lengths(page, T)
    ks, vs = odd_scales(heads[0], 1) * 40, odd_scales(heads[0], 2) * 40
    kp, vp, bt = sentinel_pool(heads[0], page, D, lens, seed=T + 1)
    ref = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, lens, ks, vs, None, None, 0)
    gk, gv, _ = run(k_new, v_new, kp, vp, bt, lens, ks, vs)
    nk, nv = report_mismatch(gk, ref.k_pages, k_new, "K"), report_mismatch(gv, ref.v_pages, v_new, "V")
    assert nk == 0 and nv == 0, (nk, nv)


@pytest.mark.parametrize("D,heads,page,T", GRID, ids=grid_ids)
def test_unit_tables_rotate_exactly(built, dev, D, heads, page, T):
    """cos = 1, sin = 0: the pools of the call without a rotation, and q_out = q. cos = 0, sin = 1: every pair becomes (-x2, x1) exactly, then
    quantised. The inputs hold no zero here: x1 0 - x2 1 gives a zero whose sign is the sum's, not the input's."""
    k_new, v_new, q = problem(D, heads, T)
    k_new, v_new = (torch.where(x == 0, torch.ones_like(x), x) for x in (k_new, v_new))
    lens = lengths(page, T)
    cap = max_pages_of(page) * page
    ks, vs = pow2_scales(heads[0]), odd_scales(heads[0], 3) * 40
    kp, vp, bt = sentinel_pool(heads[0], page, D, lens, seed=T)
    plain = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, lens, ks, vs, None, None, 0)
    one, zero = torch.ones(cap, D // 2), torch.zeros(cap, D // 2)
    for mode in (1, 2):
        gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, ks, vs, q, torch.cat((one, zero), dim=1), MODE_NAMES[mode])
        assert torch.equal(bits(gk), bits(plain.k_pages)) and torch.equal(bits(gv), bits(plain.v_pages)), mode
        assert bool((qo == q).all()), mode
        table = torch.cat((zero, one), dim=1)
        ref = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, lens, ks, vs, q, table, mode)  # (-x2, x1) in float64: exact, and exact in fp32
        gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, ks, vs, q, table, MODE_NAMES[mode])
        assert torch.equal(bits(gv), bits(plain.v_pages)), mode
        assert torch.equal(bits(gk), bits(ref.k_pages)) and not torch.equal(bits(gk), bits(plain.k_pages)), mode
        assert bool((qo.double() == ref.q_rot).all()), mode


@pytest.mark.parametrize("D,heads,page,T", GRID, ids=grid_ids)
def test_general_rotation_within_the_derived_bound(built, dev, D, heads, page, T):
    k_new, v_new, q = problem(D, heads, T)
    Hkv = heads[0]
    lens = lengths(page, T)
    table = random_table(max_pages_of(page) * page, D)
    ks, vs = odd_scales(Hkv, 4) * 40, pow2_scales(Hkv)
    kp, vp, bt = sentinel_pool(Hkv, page, D, lens, seed=T + 2)
    for mode in (1, 2):
        ref = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, lens, ks, vs, q, table, mode)
        assert len(ref.live) == B * T
        gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, ks, vs, q, table, MODE_NAMES[mode])
        assert torch.equal(bits(gv), bits(ref.v_pages)), mode
        keep = ~ref.k_live[:, None, :, None].expand_as(gk)
        assert bool((bits(gk)[keep] == SENTINEL).all()), mode
        worst, clamped = 0.0, 0
        s64 = ks.double().view(Hkv, 1)
        for (b, t) in ref.live:
            pos = int(lens[b]) - T + t
            got = f8.dequantize(gk[int(bt[b, pos // page]), :, pos % page], s64, torch.float64)
            y, mag = ref.k_rot[b, t], ref.k_mag[b, t]
            inside = y.abs() <= 448.0 * s64
            worst = max(worst, ((got - y).abs() / f8.bound(y, s64, mag))[inside].max().item())
            assert bool((got[~inside] == (448.0 * s64 * y.sign())[~inside]).all()), (mode, b, t)  # beyond the clamp: +-448 exactly
            clamped += int((~inside).sum())
        qworst = ((qo.double() - ref.q_rot).abs() / kr.bound(ref.q_rot, ref.q_mag)).max().item()
        print("D=%d H=%s page=%d T=%d %s: K worst error / bound %.4f (%d clamped), q_out %.4f" % (D, heads, page, T, MODE_NAMES[mode], worst, clamped, qworst))
        assert bool(torch.isfinite(qo).all()) and worst <= 1.0 and qworst <= 1.0, (mode, worst, qworst)


# lengths that leave tokens without a place, (Hkv, Hq) = (5, 20), page 16, three pages (48 rows)
DEAD = {
    "short": lambda T: [3, 0, -7],                       # len < T: only the last 3 tokens are live; len = 0 and len < 0: none is
    "long": lambda T: [48 + 2, 2 ** 31 - 1, -2 ** 31],   # len > capacity: the last 2 tokens are not live; the int32 extremes: none is, no overflow
    "mixed": lambda T: [48 + 4, 5, 48 + T],              # the last 4 not live; the last 5 live; the first token one past the last row
}


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("case", sorted(DEAD))
def test_tokens_without_a_place_write_nothing_and_zero_their_q_rows(built, dev, D, case):
    heads, page, T = (5, 20), 16, 17
    k_new, v_new, q = problem(D, heads, T)
    lens = DEAD[case](T)
    ks, vs = pow2_scales(5), pow2_scales(5, 1)
    kp, vp, bt = sentinel_pool(5, page, D, lens, seed=2)
    table = random_table(40, D)  # max_pos = 40 < 48: positions 40 .. 47 are not live with a rotation
    for mode in (0, 1, 2):
        ref = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, lens, ks, vs, q if mode else None, table if mode else None, mode)
        assert 0 < len(ref.live) < B * T
        gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, ks, vs, *((q, table, MODE_NAMES[mode]) if mode else ()))
        written = ref.k_live[:, None, :, None].expand_as(kp)
        assert bool((bits(gk)[~written] == SENTINEL).all()) and bool((bits(gv)[~written] == SENTINEL).all()), mode
        assert torch.equal(bits(gv), bits(ref.v_pages)) and not bool((bits(gk)[written] == SENTINEL).all()), mode
        if mode:
            dead = torch.ones(B, T, dtype=torch.bool)
            for (b, t) in ref.live:
                dead[b, t] = False
            assert bool(dead.any()) and bool((qo[dead] == 0).all()) and bool(torch.isfinite(qo).all()), mode
            assert ((qo.double() - ref.q_rot).abs() / kr.bound(ref.q_rot, ref.q_mag)).max().item() <= 1.0, mode
        else:
            assert torch.equal(bits(gk), bits(ref.k_pages))


@pytest.mark.parametrize("D", DS)
def test_an_out_of_range_table_entry_stores_nothing(built, dev, D):
    heads, page, T = (5, 5), 16, 3
    k_new, v_new, _ = problem(D, heads, T)
    lens = lengths(page, T)
    ks = vs = pow2_scales(5)
    kp, vp, bt = sentinel_pool(5, page, D, lens, seed=3)
    P = kp.shape[0]
    bad = bt.clone()
    bad[0, 0], bad[2, 2] = P, -1  # sequences 0 and 2 name no page of the pool
    ok = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, [0, lens[1], 0], ks, vs, None, None, 0)  # what sequence 1 alone writes
    gk, gv, _ = run(k_new, v_new, kp, vp, bad, lens, ks, vs)
    assert torch.equal(bits(gk), bits(ok.k_pages)) and torch.equal(bits(gv), bits(ok.v_pages))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_two_calls_give_equal_bytes_and_q_in_place_equals_out_of_place(built, dev, D, mode):
    heads, page, T = (5, 20), 16, 17
    k_new, v_new, q = problem(D, heads, T)
    lens = [17, 32, 48 + 3]
    ks, vs = odd_scales(5, 5) * 40, odd_scales(5, 6) * 40
    kp, vp, bt = sentinel_pool(5, page, D, lens, seed=8)
    args = (q, random_table(48, D), MODE_NAMES[mode]) if mode else ()
    a, b = run(k_new, v_new, kp, vp, bt, lens, ks, vs, *args), run(k_new, v_new, kp, vp, bt, lens, ks, vs, *args)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    if mode:
        assert torch.equal(a[2].view(torch.int16), b[2].view(torch.int16))
        c = run(k_new, v_new, kp, vp, bt, lens, ks, vs, *args, inplace=True)
        assert torch.equal(bits(a[0]), bits(c[0])) and torch.equal(bits(a[1]), bits(c[1])) and torch.equal(a[2].view(torch.int16), c[2].view(torch.int16))
        assert not torch.equal(c[2].view(torch.int16), q.view(torch.int16))


def test_python_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    f = pkg.kv_append_paged_fp8
    Bq, T, Hkv, Hq, page, mp, D, P = 2, 3, 2, 8, 16, 4, 64, 9
    h = lambda *s: torch.zeros(*s, dtype=torch.half, device=dev)  # noqa: E731
    p8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev).view(f8.F8)  # noqa: E731
    kn, vn, kp, vp, q, qo = h(Bq, T, Hkv, D), h(Bq, T, Hkv, D), p8(P, Hkv, page, D), p8(P, Hkv, page, D), h(Bq, T, Hq, D), h(Bq, T, Hq, D)
    bt = torch.zeros(Bq, mp, dtype=torch.int32, device=dev)
    sl = torch.zeros(Bq, dtype=torch.int32, device=dev)  # every token at a negative position: a call that gets through writes nothing
    ks, vs = torch.ones(Hkv, device=dev), torch.ones(Hkv, device=dev)
    tab = torch.zeros(64, D, device=dev)
    f(kn, vn, kp, vp, bt, sl, ks, vs)
    f(kn, vn, kp, vp, bt, sl, ks, vs, q, qo, tab, "half")
    with pytest.raises(RuntimeError, match="kv_append_paged_fp8: headdim 96 not supported"):
        f(h(Bq, T, Hkv, 96), h(Bq, T, Hkv, 96), p8(P, Hkv, page, 96), p8(P, Hkv, page, 96), bt, sl, ks, vs)
    with pytest.raises(RuntimeError, match="kv_append_paged_fp8: page size 48 not supported"):
        f(kn, vn, p8(P, Hkv, 48, D), p8(P, Hkv, 48, D), bt, sl, ks, vs)
    with pytest.raises(RuntimeError, match="kv_append_paged_fp8: rope 'neox' not supported"):
        f(kn, vn, kp, vp, bt, sl, ks, vs, q, qo, tab, "neox")
    with pytest.raises(RuntimeError, match="status -1"):
        f(kn, vn, kp, kp, bt, sl, ks, vs)  # the pools are one tensor
    bad = [
        lambda: f(kn, vn, h(P, Hkv, page, D), h(P, Hkv, page, D), bt, sl, ks, vs),    # fp16 pools
        lambda: f(kn, vn, kp, vp.view(torch.uint8), bt, sl, ks, vs),                  # a byte pool that is no e4m3 tensor
        lambda: f(kn, vn, kp, vp.view(torch.float8_e5m2), bt, sl, ks, vs),
        lambda: f(kn.float(), vn, kp, vp, bt, sl, ks, vs),
        lambda: f(kn, vn, kp, vp, bt, sl, ks.half(), vs),                             # scales: dtype, device, shape
        lambda: f(kn, vn, kp, vp, bt, sl, ks, vs.double()),
        lambda: f(kn, vn, kp, vp, bt, sl, ks.cpu(), vs),
        lambda: f(kn, vn, kp, vp, bt, sl, ks, vs.cpu()),
        lambda: f(kn, vn, kp, vp, bt, sl, ks[:1], vs),
        lambda: f(kn, vn, kp, vp, bt, sl, ks, torch.ones(Hkv, 1, device=dev)),
        lambda: f(kn, vn, kp, vp, bt, sl, ks, torch.ones(2 * Hkv, device=dev)[::2]),  # not contiguous
        lambda: f(kn, vn, kp, vp, bt.cpu(), sl, ks, vs),
        lambda: f(kn, vn, kp, vp, bt, sl.long(), ks, vs),
        lambda: f(kn, vn, kp, vp[:4].contiguous(), bt, sl, ks, vs),
        lambda: f(kn, vn, kp, vp, bt, sl, ks, vs, q, None, tab, "half"),              # the pointer rules of rope
        lambda: f(kn, vn, kp, vp, bt, sl, ks, vs, q, qo, None, "half"),
        lambda: f(kn, vn, kp, vp, bt, sl, ks, vs, rope_table=tab),
    ]
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
    torch.cuda.synchronize()
    assert bool((bits(kp) == 0).all()) and bool((bits(vp) == 0).all()) and bool((qo == 0).all())
