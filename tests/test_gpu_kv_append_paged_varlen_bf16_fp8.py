"""GPU: the packed append of bf16 rows into FP8 (e4m3) pools -- cuda_learn_notes_amd.kv_append_paged_varlen_bf16_fp8 (csrc/
kv_append_paged_varlen_bf16_fp8.cuh) -- against tests/paged_bf16_fp8_reference.ref_append: V rows and rope = none K rows are
fp8_kv_reference.quantize of the input byte for byte, rotated K rows within fp8_kv_reference.bound of the fp64 rotation, q_out within
kv_append_bf16_reference.bound, every pool byte no live token owns and every q row of no sequence bit for bit what it was (the pools' free pages
hold the NaN byte 0x7F, the rows of no sequence 2^100), dead tokens write nothing and get zero q_out rows. The packed problems, the random cos /
sin table and the lengths are those of tests/test_gpu_paged_bf16_step.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import kv_append_bf16_reference as ar  # noqa: E402
import paged_bf16_fp8_reference as fr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import prefill_varlen_reference as vr  # noqa: E402
import test_gpu_paged_bf16_step as st  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DS = [64, 128]
MODE_NAMES = st.MODE_NAMES
Q_FILL = st.Q_FILL
bits = st.bits


def pool_of(ci, D, lens, seed):
    """The quantised pool of the case: live pages hold codes, every other page 0x7F."""
    geom, _ = vr.CASES[ci]
    k, v = st.problem(ci, D)[4:]
    ks, vs = fr.scales(geom[0])
    kp, vp, bt = fr.quantize_pools(pr.make_pool(k, v, geom[2], lens, seed=seed), ks, vs)
    assert int((f8.bits(kp) == fr.NAN_BYTE).sum()) >= kp[0].numel()
    return kp, vp, bt, ks, vs


def run(k_new, v_new, kp, vp, bt, lens, cu, ks, vs, q=None, table=None, rope="none", inplace=False, dev="cuda"):
    """The call on copies of everything; returns the pools (uint8) and q_out on the CPU, after asserting that the inputs kept their bits."""
    import cuda_learn_notes_amd as pkg
    knd, vnd, kd, vd, bd, ksd, vsd = (t.to(dev) for t in (k_new, v_new, kp, vp, bt, ks, vs))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    cd = torch.tensor(list(cu), dtype=torch.int32, device=dev)
    qd = qo = td = None
    if q is not None:
        qd = q.to(dev)
        qo = qd if inplace else torch.full(qd.shape, Q_FILL, dtype=torch.int16, device=dev).view(BF)
    if table is not None:
        td = table.to(dev)
    pkg.kv_append_paged_varlen_bf16_fp8(knd, vnd, kd, vd, bd, sl, cd, ksd, vsd, qd, qo, td, rope)
    torch.cuda.synchronize()
    assert torch.equal(bits(knd.cpu()), bits(k_new)) and torch.equal(bits(vnd.cpu()), bits(v_new))
    assert torch.equal(bd.cpu(), bt) and torch.equal(ksd.cpu(), ks) and torch.equal(vsd.cpu(), vs)
    if q is not None and not inplace:
        assert torch.equal(bits(qd.cpu()), bits(q))
    return f8.bits(kd.cpu()), f8.bits(vd.cpu()), (qo.cpu() if qo is not None else None)


def check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, ks, vs, q, table, mode, page, what):
    rk, rv, k_live, rows, dead = fr.ref_append(k_new, v_new, kp, vp, bt, lens, cu, ks, vs, q, table, mode)
    assert torch.equal(gv, rv), what  # V: quantize() of the input byte for byte, every other byte unchanged
    keep = ~k_live[:, None, :, None].expand_as(gk)
    assert torch.equal(gk[keep], f8.bits(kp)[keep]) and torch.equal(gv[keep], f8.bits(vp)[keep]), what
    if mode == 0:
        assert torch.equal(gk, rk), what  # K without a rotation: byte for byte too
    worst = 0.0
    scale = ks.double().reshape(-1, 1)
    for (row, b, pos, k_rot, k_mag, q_rot, q_mag) in rows:
        got = gk[int(bt[b, pos // page]), :, pos % page]
        assert not bool((got & 0x7F == 0x7F).any()), what  # no NaN code
        if mode != 0:
            back = f8.dequantize(got.view(f8.F8), scale, torch.float64)
            worst = max(worst, ((back - k_rot).abs() / f8.bound(k_rot, scale, k_mag)).max().item())
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


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("ci", range(len(vr.CASES)), ids=st.CASE_IDS)
def test_append_every_token_live(built, dev, ci, mode, D):
    geom, T = vr.CASES[ci]
    page, Nmax = geom[2], geom[2] * geom[3]
    k_new, v_new, q, cu = st.problem(ci, D)[:4]
    lens = st.lengths(geom, T)
    kp, vp, bt, ks, vs = pool_of(ci, D, lens, ci)
    what = "fp8 append D=%d %s %s" % (D, st.CASE_IDS[ci], MODE_NAMES[mode])
    if mode == 0:
        gk, gv, _ = run(k_new, v_new, kp, vp, bt, lens, cu, ks, vs)
        rows, dead = check_reference(gk, gv, None, k_new, v_new, kp, vp, bt, lens, cu, ks, vs, None, None, 0, page, what)
        assert len(rows) == sum(T) and not dead and not torch.equal(gk, f8.bits(kp))
        again = run(k_new, v_new, kp, vp, bt, lens, cu, ks, vs)  # two runs repeat their bytes
        assert torch.equal(again[0], gk) and torch.equal(again[1], gv)
        return
    table = st.random_table(Nmax, D)
    gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, cu, ks, vs, q, table, MODE_NAMES[mode])
    rows, dead = check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, ks, vs, q, table, mode, page, what)
    assert len(rows) == sum(T) and not dead
    ak, av, none = run(k_new, v_new, kp, vp, bt, lens, cu, ks, vs, None, table, MODE_NAMES[mode])  # K alone: no q rows in the grid
    assert none is None and torch.equal(ak, gk) and torch.equal(av, gv)
    ik, iv, iq = run(k_new, v_new, kp, vp, bt, lens, cu, ks, vs, q, table, MODE_NAMES[mode], inplace=True)  # q_out is q
    assert torch.equal(ik, gk) and torch.equal(iv, gv)
    assert torch.equal(bits(iq[cu[0]:cu[-1]]), bits(qo[cu[0]:cu[-1]])) and not torch.equal(bits(iq[cu[0]:cu[-1]]), bits(q[cu[0]:cu[-1]]))
    assert torch.equal(bits(iq[:cu[0]]), bits(q[:cu[0]])) and torch.equal(bits(iq[cu[-1]:]), bits(q[cu[-1]:]))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_append_dead_tokens_write_nothing(built, dev, mode, D):
    """The dead-token case of tests/test_gpu_paged_bf16_step.py: pos < 0, a T_b = 0 sequence with a length, len = 0, pos >= max_pos and
    pos >= max_pages page; every table entry that no live token resolves through lies outside [0, P)."""
    ci = 0
    geom, T = vr.CASES[ci]
    page, Nmax = geom[2], geom[2] * geom[3]
    k_new, v_new, q, cu = st.problem(ci, D)[:4]
    lens = [7, 77, 0, 1010, Nmax + 30]
    kp, vp, bt, ks, vs = pool_of(ci, D, lens, 2)
    table = st.random_table(Nmax, D)[:1000].contiguous() if mode else None
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
    gk, gv, qo = run(k_new, v_new, kp, vp, bt, lens, cu, ks, vs, *args)
    rows, dead = check_reference(gk, gv, qo, k_new, v_new, kp, vp, bt, lens, cu, ks, vs, q if mode else None, table, mode, page,
                                 "fp8 append D=%d dead tokens %s" % (D, MODE_NAMES[mode]))
    assert len(rows) == 7 + (23 if mode else 33) + (76 if mode else 100) and len(dead) == sum(T) - len(rows)


@pytest.mark.parametrize("D", DS)
def test_append_clamps_to_the_largest_code(built, dev, D):
    """Inputs 16 x the usual under the same scales: |y| / scale passes 448 for part of the elements, which must come out as +-448 (0x7E / 0xFE),
    never as the NaN code; byte for byte quantize() of the input."""
    ci = 0
    geom, T = vr.CASES[ci]
    k_new, v_new, q, cu = st.problem(ci, D)[:4]
    big_k, big_v = (k_new.float() * 64).to(BF), (v_new.float() * 64).to(BF)
    big_k[:cu[0]], big_k[cu[-1]:], big_v[:cu[0]], big_v[cu[-1]:] = 2.0 ** 100, 2.0 ** 100, 2.0 ** 100, 2.0 ** 100
    lens = st.lengths(geom, T)
    kp, vp, bt, ks, vs = pool_of(ci, D, lens, 1)
    gk, gv, _ = run(big_k, big_v, kp, vp, bt, lens, cu, ks, vs)
    check_reference(gk, gv, None, big_k, big_v, kp, vp, bt, lens, cu, ks, vs, None, None, 0, geom[2], "fp8 append clamp D=%d" % D)
    assert int((gk & 0x7F == 0x7E).sum()) > int((f8.bits(kp) & 0x7F == 0x7E).sum())
