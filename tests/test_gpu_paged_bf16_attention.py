"""GPU: the bf16 attention entries over a paged KV cache -- cuda_learn_notes_amd.fa2_prefill_paged_varlen_bf16 (csrc/
flash_attn_prefill_paged_varlen_bf16.cuh) and fa2_decode_paged_multi_bf16 (csrc/flash_attn_decode_paged_multi_bf16.cuh) -- against the fp64
references on the bf16 inputs' exact values (prefill_varlen_reference.ref_prefill_paged_varlen, multi_decode_reference.ref_decode_paged_multi).
O is held to the emulation bound of tests/paged_bf16_reference.py, LSE to decode_reference.lse_tol; -inf LSE entries and zero rows are compared
exactly. Pools come from paged_decode_reference.make_pool (NaN poison pages, shuffled placement). Every parity case prints err / bound before it
asserts (pytest -s). A packed run and its references are computed once per (case, D, context) and shared by the tests that look at them."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import multi_decode_reference as mr  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import prefill_varlen_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DS = [64, 128]
CONTEXTS = [0, 63, 64, 200]  # keys in front of the new tokens: none, one short of the key step, the key step, several steps
FIRST, SPARE = 3, 5          # packed rows in front of cu_q[0] and behind cu_q[B]
O_FILL, L_FILL = 0x4D2B, 0x4B1DF00D  # the bit patterns the rows of no sequence must keep (a finite bf16, a finite fp32)
CASE_IDS = ["x".join(map(str, g)) for g, _ in vr.CASES]
bits = lambda t: t.view(torch.int16)  # noqa: E731
fbits = lambda t: t.view(torch.int32)  # noqa: E731


@functools.lru_cache(maxsize=None)
def problem(ci, D, k_scale=1.0, v_scale=1.0):
    """Gaussian bf16 (q_b [T_b,Hq,D] per sequence, dense k, v [B,Hkv,Nmax,D]) on the CPU, made once and never modified; the scales are powers of
    two, so the scaled tensors are exact."""
    (Hkv, G, page, mp), T = vr.CASES[ci]
    g = torch.Generator().manual_seed(97 * ci + D)
    qs = tuple(torch.randn(t, Hkv * G, D, generator=g).to(BF) for t in T)
    k, v = (torch.randn(len(T), Hkv, page * mp, D, generator=g).to(BF) for _ in range(2))
    return qs, (k.float() * k_scale).to(BF), (v.float() * v_scale).to(BF)


def pack(qs, first=FIRST, spare=SPARE):
    """(q [total_q,Hq,D], cu): the sequences packed from row `first` on; the rows of no sequence hold 2^100 -- read into a product, they would show."""
    cu = vr.cu_of([x.shape[0] for x in qs], first)
    q = torch.full((cu[-1] + spare,) + tuple(qs[0].shape[1:]), 2.0 ** 100, dtype=BF)
    for b, x in enumerate(qs):
        q[cu[b]:cu[b + 1]] = x
    return q, cu


def run_prefill(q, kp, vp, bt, lens, cu, dev="cuda"):
    import cuda_learn_notes_amd as pkg
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:2], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    pkg.fa2_prefill_paged_varlen_bf16(qd, kd, vd, bd, sl, cd, o, lse)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def check(o, lse, ro, rl, emul, what):
    """O within the emulation bound, LSE within lse_tol, -inf LSE entries and their zero rows exactly. Returns err / bound of O."""
    assert bool(torch.isfinite(o).all()), what
    bo = br.o_bound(emul, ro)
    eo = (o.double() - ro).abs().max().item()
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float("-inf")).all()), what
    assert bool((o[~fin] == 0).all()), what  # a query that sees no key
    el = (lse.double()[fin] - rl[fin]).abs().max().item() if bool(fin.any()) else 0.0
    bl = dr.lse_tol(rl)
    print("%s: O err %.3e / bound %.3e = %.4f   LSE err %.3e / bound %.3e = %.4f" % (what, eo, bo, eo / bo, el, bl, el / bl))
    assert eo <= bo, (what, eo, bo)
    assert el <= bl, (what, el, bl)
    return eo / bo


@functools.lru_cache(maxsize=None)
def packed_run(ci, D, ctx, k_scale=1.0, v_scale=1.0):
    """One packed call with `ctx` keys in front of every sequence's new tokens (fewer where the cache is full), its pool and its references."""
    (Hkv, G, page, mp), T = vr.CASES[ci]
    qs, k, v = problem(ci, D, k_scale, v_scale)
    q, cu = pack(qs)
    lens = [min(ctx, page * mp - t) + t for t in T]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=ctx)
    o, lse = run_prefill(q, kp, vp, bt, lens, cu)
    ro, rl = vr.ref_prefill_paged_varlen(q, kp, vp, bt, lens, cu)
    emul = br.emul_prefill_paged_varlen(q, kp, vp, bt, lens, cu)
    return dict(q=q, cu=cu, lens=lens, pool=(kp, vp, bt), o=o, lse=lse, ro=ro, rl=rl, emul=emul, qs=qs)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("ci", range(len(vr.CASES)), ids=CASE_IDS)
def test_prefill_parity_and_untouched_rows(built, dev, ci, D):
    """T_b = 0, 1, 129, 130, G = 1 .. 8, pages 16 .. 256, with 0, 63, 64 and 200 keys in front: O and LSE against the fp64 reference, and the packed
    rows outside [cu_q[0], cu_q[B]) keep the bit pattern they were filled with."""
    for ctx in CONTEXTS:
        r = packed_run(ci, D, ctx)
        cu = r["cu"]
        for sl in (slice(0, cu[0]), slice(cu[-1], None)):
            assert bool((bits(r["o"][sl]) == O_FILL).all()) and bool((fbits(r["lse"][sl]) == L_FILL).all()), (ci, D, ctx)
        seq = slice(cu[0], cu[-1])
        check(r["o"][seq], r["lse"][seq], r["ro"][seq], r["rl"][seq], r["emul"][seq], "prefill D=%d %s ctx=%d lens=%s" % (D, CASE_IDS[ci], ctx, r["lens"]))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("ci", range(len(vr.CASES)), ids=CASE_IDS)
def test_prefill_sequence_does_not_depend_on_its_neighbours(built, dev, ci, D):
    """Every sequence of every packed run above, called alone with B = 1: the same bits, O and LSE."""
    for ctx in CONTEXTS:
        r = packed_run(ci, D, ctx)
        kp, vp, bt = r["pool"]
        cu = r["cu"]
        for b, qb in enumerate(r["qs"]):
            t = qb.shape[0]
            q1 = torch.cat((qb, torch.full((1,) + tuple(qb.shape[1:]), 2.0 ** 100, dtype=BF)))  # one spare row: total_q >= 1 also for T_b = 0
            o1, l1 = run_prefill(q1, kp, vp, bt[b:b + 1].contiguous(), [r["lens"][b]], [0, t])
            assert torch.equal(bits(o1[:t]), bits(r["o"][cu[b]:cu[b + 1]])) and torch.equal(fbits(l1[:t]), fbits(r["lse"][cu[b]:cu[b + 1]])), (ci, D, ctx, b)
            assert bool((bits(o1[t:]) == O_FILL).all())


@pytest.mark.parametrize("D", DS)
def test_prefill_range_v_at_two_to_the_17(built, dev, D):
    """V scaled by 2^17 and K by 2^4: no fp16 can hold these inputs; O is finite and within the bound of this case's own reference."""
    r = packed_run(0, D, 64, 16.0, 2.0 ** 17)
    assert float(r["pool"][1][torch.isfinite(r["pool"][1])].abs().max()) > 65504.0
    seq = slice(r["cu"][0], r["cu"][-1])
    assert float(r["ro"][seq].abs().max()) > 65504.0
    check(r["o"][seq], r["lse"][seq], r["ro"][seq], r["rl"][seq], r["emul"][seq], "prefill range D=%d" % D)


def test_prefill_repeats_its_bits(built, dev):
    r = packed_run(0, 128, 63)
    o, lse = run_prefill(r["q"], *r["pool"], r["lens"], r["cu"])
    assert torch.equal(bits(o), bits(r["o"])) and torch.equal(fbits(lse), fbits(r["lse"]))


# ---------------------------------------------------------------------------------------------------- multi-token decode

PAGE = 16


def multi_lens(T):
    return [0, 1, T - 1, 127, 128, 129, 300]


@functools.lru_cache(maxsize=None)
def multi_problem(B, T, Hkv, G, Nmax, D, k_scale=1.0, v_scale=1.0):
    g = torch.Generator().manual_seed(1000 * T + 10 * G + D + B)
    q = torch.randn(B, T, Hkv * G, D, generator=g).to(BF)
    k, v = (torch.randn(B, Hkv, Nmax, D, generator=g).to(BF) for _ in range(2))
    return q, (k.float() * k_scale).to(BF), (v.float() * v_scale).to(BF)


def run_multi(q, kp, vp, bt, lens, exact_workspace=False, dev="cuda"):
    """The call on copies; with exact_workspace a caller's workspace of exactly the planned bytes in front of a guard band that must stay intact."""
    import cuda_learn_notes_amd as pkg
    qd, kd, vd, bd = (t.to(dev) for t in (q, kp, vp, bt))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full(qd.shape, O_FILL, dtype=torch.int16, device=dev).view(BF)
    lse = torch.full(qd.shape[:3], L_FILL, dtype=torch.int32, device=dev).view(torch.float32)
    ws = None
    if exact_workspace:
        B, T, Hq, D = q.shape
        need = pkg.fa2_decode_paged_multi_bf16_plan(B, T, Hq, kp.shape[1], bt.shape[1], kp.shape[2], D)[2]
        assert need > 0
        buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        ws = buf[:need]
    pkg.fa2_decode_paged_multi_bf16(qd, kd, vd, bd, sl, o, lse, ws)
    torch.cuda.synchronize()
    if exact_workspace:
        assert bool((buf[need:] == 0xA5).all()), "the guard band behind the workspace"
    return o.cpu(), lse.cpu()


def multi_case(q, k, v, lens, what, exact_workspace=False, seed=0):
    kp, vp, bt = pr.make_pool(k, v, PAGE, lens, seed=seed)
    o, lse = run_multi(q, kp, vp, bt, lens, exact_workspace)
    ro, rl = mr.ref_decode_paged_multi(q, kp, vp, bt, lens)
    ratio = check(o, lse, ro, rl, br.emul_decode_paged_multi(q, kp, vp, bt, lens), what)
    return o, lse, (kp, vp, bt), ratio


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_multi_parity_one_split(built, dev, T, G, D):
    """Lengths 0, 1, T - 1, 127, 128, 129 and 300 on pages of 16: empty sequences, sequences shorter than their T, both sides of the 128-key step."""
    import cuda_learn_notes_amd as pkg
    lens = multi_lens(T)
    B, Hkv, Nmax = len(lens), 2, 304
    assert pkg.fa2_decode_paged_multi_bf16_plan(B, T, Hkv * G, Hkv, Nmax // PAGE, PAGE, D)[0] == 1
    q, k, v = multi_problem(B, T, Hkv, G, Nmax, D)
    multi_case(q, k, v, lens, "multi D=%d T=%d G=%d lens=%s" % (D, T, G, lens))


@pytest.mark.parametrize("D", DS)
def test_multi_parity_split_over_the_keys_with_a_callers_workspace(built, dev, D):
    """max_pages page = 4096 with one KV head: 16 splits of 256 keys. Lengths that fill the last split (4096), that end on a split's last key (1024:
    12 splits empty), one past it (257: one key in the second split), inside the first (100), and 0; the workspace is the caller's, exactly the
    planned bytes, with a guard band behind it."""
    import cuda_learn_notes_amd as pkg
    T, G, Hkv, Nmax = 2, 2, 1, 4096  # few query rows: the fp64 reference copies the cache once per query token and head
    lens = [4096, 1024, 257, 100, 0]
    S, C, ws = pkg.fa2_decode_paged_multi_bf16_plan(len(lens), T, Hkv * G, Hkv, Nmax // PAGE, PAGE, D)
    assert S > 1 and (S, C) == (16, 256) and ws == len(lens) * T * Hkv * G * S * (D + 2) * 4
    assert pkg.fa2_decode_paged_multi_bf16_plan(1, 1, 1, 1, Nmax // PAGE, PAGE, D)[0] > 1  # B = 1, Hkv = 1 alone splits too
    q, k, v = multi_problem(len(lens), T, Hkv, G, Nmax, D)
    o, lse, pool, _ = multi_case(q, k, v, lens, "multi split D=%d lens=%s" % (D, lens), exact_workspace=True)
    o2, lse2 = run_multi(q, *pool, lens)  # the wrapper's own workspace: the same bits, and the same bits twice
    assert torch.equal(bits(o), bits(o2)) and torch.equal(fbits(lse), fbits(lse2))


@pytest.mark.parametrize("D", DS)
def test_multi_range_v_at_two_to_the_17(built, dev, D):
    """V scaled by 2^17 and K by 2^4, one split and sixteen."""
    for (T, G, Hkv, Nmax, lens) in ((3, 4, 2, 304, multi_lens(3)), (2, 2, 1, 4096, [4096, 300])):
        q, k, v = multi_problem(len(lens), T, Hkv, G, Nmax, D, 16.0, 2.0 ** 17)
        o, _, _, _ = multi_case(q, k, v, lens, "multi range D=%d Nmax=%d" % (D, Nmax), seed=1)
        assert float(o.float().abs().max()) > 65504.0
