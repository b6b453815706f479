"""GPU: fa2_decode_paged_mla_sparse_bf16_fp8 over a pool of more than 2^32 elements: the e4m3 [P, 16, 576] view of the 8 GiB buffer of
tests/test_gpu_paged_mla_large_pool.py, planned by tests/paged_mla_large_pool.py. The kernel forms the row address
((pg << page_shift) + (idx & pmask)) 576 + 16 g4 bytes behind a (size_t) cast of its own (csrc/flash_attn_decode_paged_mla_sparse_bf16_fp8.cuh)
that no other test holds up.

The oracle adds no tolerance. A case of the family's builders runs on its small pool and is held to the reference by the family's check; its
live pages are then copied on the device to the named pages of the large view -- on both sides of element 2^31, 2^32, 2^33 and at the end of
the pool, the high pages going to table entries that a valid slot lists --, the table is remapped, the dead entries point at a poison page, and
the entry runs again under both orders of the plan: O and LSE keep every bit and are finite. A wrapped offset reads NaN poison."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_all_entries as ae  # noqa: E402
import paged_mla_fp8_reference as mf  # noqa: E402
import paged_mla_large_pool as mlp  # noqa: E402
import paged_mla_sparse_fp8_reference as s8  # noqa: E402
import test_gpu_paged_mla_large_pool as lp  # noqa: E402

pytestmark = pytest.mark.gpu

buffer = lp.buffer  # the module-scoped 8 GiB byte buffer, allocated once for this module
KVS, PAGE, DEV = lp.KVS, lp.PAGE, "cuda"


def run(q, pool, bt, lens, idx):
    c = lp.pkg()
    B, T, Hq, _ = q.shape
    o = torch.full((B, T, Hq, lp.DC), lp.O_FILL, dtype=torch.int16, device=DEV).view(lp.BF)
    lse = torch.full((B, T, Hq), lp.L_FILL, dtype=torch.int32, device=DEV).view(torch.float32)
    need = c.fa2_decode_paged_mla_sparse_bf16_fp8_plan(B, T, Hq, idx.shape[2], bt.shape[1], PAGE)
    ws = torch.empty(max(need[2], 16), dtype=torch.uint8, device=DEV)
    c.fa2_decode_paged_mla_sparse_bf16_fp8(q, pool, bt, lp.i32(lens), mf.scale_t(KVS).to(DEV), idx, lp.SCALE, o, lse, ws)
    torch.cuda.synchronize()
    return o, lse, need[0]


@pytest.mark.parametrize("case", lp.SPARSE_CASES, ids=lambda c: "T%dxHq%d%s" % (c[0], c[1], "-split" if c[2] else ""))
def test_sparse_fp8_decode_keeps_every_bit_when_its_pages_move_past_two_to_the_32(built, dev, buffer, case):
    T, Hq, split = case
    q, lens, (pool, bt) = s8.split_case(T, Hq, KVS) if split else s8.one_case(T, Hq, PAGE, KVS)
    idx = s8.split_indices(T, Hq, False) if split else s8.one_indices(T, Hq, PAGE, 200)
    what = "mla sparse fp8 decode T=%d Hq=%d%s" % (T, Hq, " split" if split else "")
    qd, pd, xd = q.to(DEV), pool.to(DEV), idx.to(DEV)
    o, lse, S = run(qd, pd, bt.to(DEV), lens, xd)
    assert (S > 1) == split, (what, S)
    lp.check(o.cpu(), lse.cpu(), *s8.decode_sparse(q, pool, bt, lens, idx, KVS, lp.SCALE), what + ", small pool")
    big = lp.Large(buffer, lp.F8)
    assert big.s == 1 and big.pool.numel() > 2 ** 33
    live = ae.live_entries(bt, lens, PAGE)
    first = lp.listed_entries(idx, bt, lens, T)
    for top_first in lp.ORDERS:
        plan = mlp.plan(big.E, big.s, len(live), seed=T + Hq, top_first=top_first)
        assert len(first) >= len(plan["must"])  # the high pages go to entries the kernel reads
        bt2, pairs, got = lp.relocate(big, pd, bt, lens, plan, first=first[:len(plan["must"])])
        assert got == set(plan["must"])
        o2, lse2, _ = run(qd, big.pool, bt2, lens, xd)
        lp.report("%s, %s" % (what, "top first" if top_first else "low first"), big, plan, [n for _, n in pairs])
        assert bool(torch.isfinite(o2.float()).all()) and not bool(torch.isnan(lse2).any()), what
        assert torch.equal(lp.bits(o2), lp.bits(o)) and torch.equal(lp.fbits(lse2), lp.fbits(lse)), what
        assert big.still_poison(plan["poison"][:4] + plan["poison"][-4:])
