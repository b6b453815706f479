"""GPU: fa2_decode_paged_mla_sparse_bf16_fp8 with the operands its host check admits at 4-byte alignment actually AT 4-byte alignment
(data_ptr() % 16 == 4): block_table, seqlens, kv_scale and indices (fa2d::check_pointers with two 16-byte inputs in front:
csrc/flash_attn_decode_paged_mla_sparse_bf16_fp8.hip; lse stays at 16 bytes and is not shifted). The surface test shows that the host accepts
such pointers; here the kernel loads through them. Each shifted operand is a copy at base + 4 bytes of a 16-byte aligned buffer
(tests/test_gpu_paged_unaligned_operands.py: shifted). A run with all four shifted, and one run per operand shifted alone, must give the bits
of the aligned run, which is first held to the reference by the family's check."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_mla_fp8_reference as mf  # noqa: E402
import paged_mla_sparse_fp8_reference as s8  # noqa: E402
import test_gpu_paged_mla_unaligned_operands as um  # noqa: E402

pytestmark = pytest.mark.gpu

KVS = mf.KV_SCALES[1]
OPERANDS = ["bt", "sl", "kvs", "idx"]
DEV = "cuda"


@pytest.mark.parametrize("split", [False, True], ids=["one-split", "several-splits"])
def test_sparse_fp8_decode_with_operands_at_4_byte_alignment(built, dev, split):
    """(3, 5) at topk 200 with one split; (2, 40) at topk 2048 with several."""
    c = um.pkg()
    T, Hq = (2, 40) if split else (3, 5)
    q, lens, (pool, bt) = s8.split_case(T, Hq, KVS) if split else s8.one_case(T, Hq, um.PAGE, KVS)
    idx = s8.split_indices(T, Hq, True) if split else s8.one_indices(T, Hq, um.PAGE, 200)
    ref = s8.decode_sparse(q, pool, bt, lens, idx, KVS, um.SCALE)
    B = len(lens)
    d = dict(q=q.to(DEV), pool=pool.to(DEV), bt=bt.to(DEV), sl=um.i32(lens), kvs=mf.scale_t(KVS).to(DEV), idx=idx.to(DEV))
    S, _, need = c.fa2_decode_paged_mla_sparse_bf16_fp8_plan(B, T, Hq, idx.shape[2], bt.shape[1], um.PAGE)
    assert (S > 1) == split
    base = None
    for which in um.variants(OPERANDS):
        x = um.with_shifts(d, which)
        o = torch.full((B, T, Hq, um.DC), um.O_FILL, dtype=torch.int16, device=DEV).view(um.BF)
        lse = torch.full((B, T, Hq), um.L_FILL, dtype=torch.int32, device=DEV).view(torch.float32)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
        assert all(x[n].data_ptr() % 16 == 4 for n in which) and lse.data_ptr() % 16 == 0
        c.fa2_decode_paged_mla_sparse_bf16_fp8(x["q"], x["pool"], x["bt"], x["sl"], x["kvs"], x["idx"], um.SCALE, o, lse, ws)
        torch.cuda.synchronize()
        got = (o.cpu(), lse.cpu())
        if base is None:
            base = got
            r = um.check(*got, *ref, "mla sparse fp8 decode T=%d Hq=%d S=%d, aligned" % (T, Hq, S))
            print("mla sparse fp8 decode S=%d: aligned run err / bound %.4f; shifting %s" % (S, r, OPERANDS))
        assert torch.equal(um.bits(got[0]), um.bits(base[0])) and torch.equal(um.fbits(got[1]), um.fbits(base[1])), (split, which)
