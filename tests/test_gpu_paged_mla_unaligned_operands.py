"""GPU: every entry of the multi-head latent attention path with the operands its host check admits at 4-byte alignment actually AT 4-byte
alignment (data_ptr() % 16 == 4). The lists are read off the host checks: block_table and seqlens of the three decode entries, kv_scale of the
e4m3 one and indices of the sparse one (fa2d::check_pointers with two 16-byte inputs in front: csrc/flash_attn_decode_paged_mla_*.hip; their lse
stays at 16 bytes and is not shifted); block_table, seqlens, cu_q, the rope table and kv_scale of the appends (csrc/kv_append_paged_mla_*.hip);
block_table, cu_k, starts and kv_scale of the gathers (csrc/kv_gather_paged_mla_*.hip); cu_q, cu_k and lse of the prefill
(paged::mla_prefill_args); lse_a, lse_b and lse of the merge (csrc/attn_merge_states_bf16.hip). The surface tests show that the host accepts such
pointers; here the kernels load through them -- the append reads the rope table as 16-byte vectors of a type that promises 4-byte alignment only
(kva::f4u), the sparse kernel's index fetch has no sibling.

Each shifted operand is a copy at base + 4 bytes of a 16-byte aligned buffer (tests/test_gpu_paged_unaligned_operands.py: shifted, shifted_lse).
A run with all of them shifted, and one run per operand shifted alone, must give the bits of the aligned run, which is first held to the family's
reference where the family has a check for the case. The call succeeding is the proof that the host accepts the operand. A shifted lse lies
inside a larger filled buffer whose words on either side keep their fill."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import mla_prefill_reference as mp  # noqa: E402
import paged_mla_fp8_reference as mf  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_gpu_mla_prefill as gp  # noqa: E402
import test_gpu_paged_mla as gm  # noqa: E402
import test_gpu_paged_mla_fp8 as gf  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402
import test_gpu_paged_unaligned_operands as ua  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F8 = torch.bfloat16, f8.F8
DC, DR, DK, SCALE, PAGE = ml.DC, ml.DR, ml.DK, ml.SCALE, 16
KVS = mf.KV_SCALES[1]
O_FILL, L_FILL, Q_FILL = sk.O_FILL, sk.L_FILL, 0x3C5A
LSE_FILL = ua.LSE_FILL
shifted, shifted_lse = ua.shifted, ua.shifted_lse
bits, fbits, check = sk.bits, sk.fbits, sk.check
DEV = "cuda"


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def variants(names):
    """No operand shifted, all of them, each alone."""
    return [[]] + [list(names)] + [[n] for n in names]


def with_shifts(d, which):
    assert all(d[n].data_ptr() % 16 == 0 for n in d if d[n] is not None)
    out = dict(d)
    for n in which:
        out[n] = shifted(d[n])
    return out


# ---------------------------------------------------------------------------------------------------- decode

DECODE_OPERANDS = {"bf16": ["bt", "sl"], "fp8": ["bt", "sl", "kvs"], "sparse": ["bt", "sl", "idx"]}


def decode_case(family, T, Hq, split):
    if family == "sparse":
        q, lens, (pool, bt) = sp.split_case(T, Hq) if split else sp.one_case(T, Hq, PAGE)
        idx = sp.split_indices(T, Hq, True) if split else sp.one_indices(T, Hq, PAGE, 200)
        return q, lens, pool, bt, idx, sp.decode_sparse(q, pool, bt, lens, idx, SCALE)
    if family == "fp8":
        q, lens, (pool, bt) = mf.split_case(T, Hq, KVS) if split else mf.one_case(T, Hq, PAGE, KVS)
        return q, lens, pool, bt, None, mf.decode(q, pool, bt, lens, KVS, SCALE)
    q, lens, (pool, bt) = ml.split_case(T, Hq) if split else ml.one_case(T, Hq, PAGE)
    return q, lens, pool, bt, None, ml.decode(q, pool, bt, lens, SCALE)


@pytest.mark.parametrize("split", [False, True], ids=["one-split", "several-splits"])
@pytest.mark.parametrize("family", ["bf16", "fp8", "sparse"])
def test_decode_with_operands_at_4_byte_alignment(built, dev, family, split):
    """(3, 5) with one split; (2, 40) with several, whose combine reads seqlens."""
    c = pkg()
    T, Hq = (2, 40) if split else (3, 5)
    q, lens, pool, bt, idx, ref = decode_case(family, T, Hq, split)
    B = len(lens)
    d = dict(q=q.to(DEV), pool=pool.to(DEV), bt=bt.to(DEV), sl=i32(lens), kvs=mf.scale_t(KVS).to(DEV) if family == "fp8" else None,
             idx=idx.to(DEV) if idx is not None else None)
    if family == "sparse":
        S, _, need = c.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, idx.shape[2], bt.shape[1], PAGE)
    else:
        S, _, need = getattr(c, "fa2_decode_paged_mla_bf16%s_plan" % ("_fp8" if family == "fp8" else ""))(B, T, Hq, bt.shape[1], PAGE)
    assert (S > 1) == split
    base = None
    for which in variants(DECODE_OPERANDS[family]):
        x = with_shifts(d, which)
        o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=DEV).view(BF)
        lse = torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=DEV).view(torch.float32)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
        assert all(x[n].data_ptr() % 16 == 4 for n in which) and lse.data_ptr() % 16 == 0
        if family == "sparse":
            c.fa2_decode_paged_mla_sparse_bf16(x["q"], x["pool"], x["bt"], x["sl"], x["idx"], SCALE, o, lse, ws)
        elif family == "fp8":
            c.fa2_decode_paged_mla_bf16_fp8(x["q"], x["pool"], x["bt"], x["sl"], x["kvs"], SCALE, o, lse, ws)
        else:
            c.fa2_decode_paged_mla_bf16(x["q"], x["pool"], x["bt"], x["sl"], SCALE, o, lse, ws)
        torch.cuda.synchronize()
        got = (o.cpu(), lse.cpu())
        if base is None:
            base = got
            r = check(*got, *ref, "mla %s decode T=%d Hq=%d S=%d, aligned" % (family, T, Hq, S))
            print("mla %s decode S=%d: aligned run err / bound %.4f; shifting %s" % (family, S, r, DECODE_OPERANDS[family]))
        assert torch.equal(bits(got[0]), bits(base[0])) and torch.equal(fbits(got[1]), fbits(base[1])), (family, split, which)


# ---------------------------------------------------------------------------------------------------- append

@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_append_with_operands_at_4_byte_alignment(built, dev, fp8):
    c = pkg()
    lens, pool, bt, cu, c_new, k_pe, q = (gf if fp8 else gm)._append_problem()
    table = c.kv_append_rope_table(gm.APPEND_NMAX, DR)
    fixed = tuple(t.to(DEV) for t in (c_new, k_pe, q))
    d = dict(bt=bt.to(DEV), sl=i32(lens), cu=i32(cu), table=table.to(DEV), kvs=mf.scale_t(KVS).to(DEV) if fp8 else None)
    for rope in ("none", "half", "interleaved"):
        names = ["bt", "sl", "cu"] + (["kvs"] if fp8 else []) + (["table"] if rope != "none" else [])
        base = None
        for which in variants(names):
            x = with_shifts(d, which)
            pl = pool.to(DEV)
            qo = torch.full(q.shape, Q_FILL, dtype=torch.int16, device=DEV).view(BF)
            tb = x["table"] if rope != "none" else None
            assert all(x[n].data_ptr() % 16 == 4 for n in which)
            if fp8:
                c.kv_append_paged_mla_bf16_fp8(*fixed[:2], pl, x["bt"], x["sl"], x["cu"], x["kvs"], fixed[2], qo, tb, rope)
            else:
                c.kv_append_paged_mla_bf16(*fixed[:2], pl, x["bt"], x["sl"], x["cu"], fixed[2], qo, tb, rope)
            torch.cuda.synchronize()
            got = (pl.view(torch.uint8).cpu(), bits(qo).cpu())
            if base is None:
                base = got
                assert not torch.equal(base[0], pool.view(torch.uint8))  # rows were written
                assert bool(torch.isfinite(qo[cu[0]:cu[-1]].float()).all())
                print("mla %s append rope=%s: shifting %s" % ("e4m3" if fp8 else "bf16", rope, names))
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (fp8, rope, which)


# ---------------------------------------------------------------------------------------------------- gather

@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_gather_with_operands_at_4_byte_alignment(built, dev, fp8):
    c = pkg()
    if fp8:
        _, lens, (pool, bt) = mf.split_case(1, 16, KVS)
        starts, counts = [990, 17, 250, 0, 0], [50, 100, 7, 100, 0]
    else:
        pool, bt = gp._gather_problem(PAGE)
        starts, counts = [0, 7, 64], [100, 30, 256 - 64 + 20]
    cu = mp.cu_of(counts, 2)
    total = cu[-1] + 3
    d = dict(pool=pool.to(DEV), bt=bt.to(DEV), cu=i32(cu), starts=i32(starts), kvs=mf.scale_t(KVS).to(DEV) if fp8 else None)
    names = ["bt", "cu", "starts"] + (["kvs"] if fp8 else [])
    base = None
    for which in variants(names):
        x = with_shifts(d, which)
        out = torch.full((total, DK), Q_FILL, dtype=torch.int16, device=DEV).view(BF)
        assert all(x[n].data_ptr() % 16 == 4 for n in which)
        if fp8:
            c.kv_gather_paged_mla_bf16_fp8(x["pool"], x["bt"], x["cu"], x["kvs"], out, x["starts"])
        else:
            c.kv_gather_paged_mla_bf16(x["pool"], x["bt"], x["cu"], out, x["starts"])
        torch.cuda.synchronize()
        got = bits(out).cpu()
        if base is None:
            base = got
            assert not bool((base[cu[0]:cu[-1]] == Q_FILL).all(dim=1).any()) and bool((base[:cu[0]] == Q_FILL).all())
            print("mla %s gather: shifting %s" % ("e4m3" if fp8 else "bf16", names))
        assert torch.equal(got, base), (fp8, which)


# ---------------------------------------------------------------------------------------------------- prefill

@pytest.mark.parametrize("causal", [True, False], ids=["causal", "non-causal"])
def test_prefill_with_operands_at_4_byte_alignment(built, dev, causal):
    c = pkg()
    Hq = 3
    q, kv, k_pe, cu_q, cu_k = mp.packed_case(tuple(mp.RAGGED_T), tuple(mp.RAGGED_L), Hq, seed=1, front=mp.FRONT, back=mp.BACK)
    tq = q.shape[0]
    seq = slice(cu_q[0], cu_q[-1])
    d = dict(q=q.to(DEV), kv=kv.to(DEV), k_pe=k_pe.to(DEV), cu_q=i32(cu_q), cu_k=i32(cu_k))
    base = None
    for which in variants(["cu_q", "cu_k", "lse"]):
        x = with_shifts(d, [n for n in which if n != "lse"])
        o = torch.full((tq, Hq, mp.DV), O_FILL, dtype=torch.int16, device=DEV).view(BF)
        lse, buf = shifted_lse((tq, Hq), DEV) if "lse" in which else (torch.full((tq, Hq), LSE_FILL, dtype=torch.int32, device=DEV).view(torch.float32), None)
        c.fa2_prefill_varlen_mla_bf16(x["q"], x["kv"], x["k_pe"], x["cu_q"], x["cu_k"], SCALE, o, lse, causal)
        torch.cuda.synchronize()
        got = (o.cpu(), lse.cpu())
        if base is None:
            base = got
            ref = mp.prefill(q, kv, k_pe, cu_q, cu_k, SCALE, causal)
            r = gp.check_rows(got, ref, seq, "mla prefill packed causal=%d, aligned" % causal)
            print("mla prefill causal=%d: aligned run err / bound %.4f; shifting cu_q, cu_k, lse" % (causal, r))
        assert torch.equal(bits(got[0]), bits(base[0])) and torch.equal(fbits(got[1]), fbits(base[1])), (causal, which)
        if buf is not None:
            assert bool((buf[:1] == LSE_FILL).all()) and bool((buf[1 + tq * Hq:] == LSE_FILL).all()), (causal, which)
            assert bool((fbits(lse[:cu_q[0]]) == LSE_FILL).all()) and bool((fbits(lse[cu_q[-1]:]) == LSE_FILL).all())  # the rows of no sequence


# ---------------------------------------------------------------------------------------------------- merge

@pytest.mark.parametrize("D", [128, 512])
def test_merge_with_operands_at_4_byte_alignment(built, dev, D):
    c = pkg()
    rows = mp.MERGE_ROWS[-1]
    g = torch.Generator().manual_seed(D + rows)
    o_a, o_b = (torch.randn(rows, D, generator=g).to(BF) for _ in range(2))
    lse_a, lse_b = (torch.randn(rows, generator=g) * 3 for _ in range(2))
    lse_a[3], lse_b[5], lse_a[7], lse_b[7] = (float("-inf"),) * 4
    ro, rl = mp.merge(o_a, lse_a, o_b, lse_b)
    d = dict(o_a=o_a.to(DEV), o_b=o_b.to(DEV), lse_a=lse_a.to(DEV), lse_b=lse_b.to(DEV))
    base = None
    for which in variants(["lse_a", "lse_b", "lse"]) + [["in-place"], ["in-place", "lse_a", "lse_b"]]:
        x = with_shifts(d, [n for n in which if n in d])
        o = torch.full((rows, D), O_FILL, dtype=torch.int16, device=DEV).view(BF)
        buf = None
        if "in-place" in which:  # lse is lse_a
            la = x["lse_a"].clone() if "lse_a" not in which else x["lse_a"]
            assert la.data_ptr() % 16 == (4 if "lse_a" in which else 0)
            c.attn_merge_states_bf16(x["o_a"], la, x["o_b"], x["lse_b"], o, la)
            lse = la
        else:
            lse, buf = shifted_lse((rows,), DEV) if "lse" in which else (torch.full((rows,), LSE_FILL, dtype=torch.int32, device=DEV).view(torch.float32), None)
            c.attn_merge_states_bf16(x["o_a"], x["lse_a"], x["o_b"], x["lse_b"], o, lse)
        torch.cuda.synchronize()
        got = (o.cpu(), lse.cpu())
        if base is None:
            base = got
            ratio = float(((got[0].double() - ro).abs() / mp.merge_bound(ro, o_a, o_b).clamp(min=1e-300)).max())
            print("merge D=%d rows=%d: aligned run O err / bound %.4f; shifting lse_a, lse_b, lse and lse is lse_a" % (D, rows, ratio))
            assert ratio <= 1.0 and torch.equal(torch.isfinite(got[1]), torch.isfinite(rl))
        assert torch.equal(bits(got[0]), bits(base[0])) and torch.equal(fbits(got[1]), fbits(base[1])), (D, which)
        if buf is not None:
            assert bool((buf[:1] == LSE_FILL).all()) and bool((buf[1 + rows:] == LSE_FILL).all()), (D, which)
