"""GPU: the two entries of the DSA indexer's FP8 cache -- mla_index_logits_paged_bf16_fp8 and kv_append_paged_index_bf16_fp8 --
over a pool whose bytes pass 2^32. Both form the page's byte offset pg (132 << page_shift) and, behind it, two address paths -- the code row
at 128 r and the scale at 128 page + 4 r -- in size_t; no other test holds those casts up: the largest FP8 index pool elsewhere is a few
hundred KiB.

The pool is the uint8 [P, 16, 132] view of the 8 GiB buffer of tests/test_gpu_paged_mla_large_pool.py, 16 bytes in: 2112 bytes a page,
P = 4 067 234 pages, so the view ends past byte 2^33. The plan is tests/mla_index_fp8_reference.large_plan (proven on the CPU by
tests/test_mla_index_fp8_surface.py): named pages at P - 1 and, for each of bytes 2^31 and 2^32, the page that holds the byte, the one above
and the one below; 0xFF poison (a NaN code, a NaN scale) on every 32-bit wrap image of a named page -- listed directly: 2112 is no power of
two, so an image is a run of bytes inside one or two pages --, on its neighbours and on pages 0 .. 7.

The oracle adds no tolerance. Logits: a parity case of tests/test_gpu_mla_index_fp8.py runs on its small pool and is held to the fp64
reference; its live pages are copied on the device to the named pages, the table is remapped, the dead entries point at a poison page, and
the entry runs again: the logits keep every bit and are finite, every poison page still holds poison. Every live page is read (the last
token sees the whole sequence). Append: both pools start from poison; afterwards every named page of the large view equals its page of the
small pool byte for byte, the pages written are exactly P - 1 and the three around each boundary, and the poison pages hold poison.

The module is skipped only on a device with less than 16 GiB in all (the imported fixture); a failed allocation is an error."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mla_index_fp8_reference as x8  # noqa: E402
import paged_all_entries as ae  # noqa: E402
import test_gpu_mla_index_fp8 as g8  # noqa: E402
import test_gpu_paged_mla_large_pool as lp  # noqa: E402

pytestmark = pytest.mark.gpu

buffer = lp.buffer  # the module-scoped 8 GiB byte buffer, allocated once for this module
U8, DEV, PAGE = torch.uint8, "cuda", x8.LARGE_PAGE


class IndexFp8Large(lp.Large):
    """The [P, 16, 132] uint8 view of the buffer; poison is the byte 0xFF."""

    def __init__(self, bufs):
        self.dtype, self.s, self.E = U8, 1, x8.LARGE_PB
        self.PB, self.P = x8.LARGE_PB, x8.large_pages()
        self.buf = bufs[0]
        assert x8.LARGE_BASE + self.P * self.PB <= x8.LARGE_BUF_BYTES == self.buf.numel() < x8.LARGE_BASE + (self.P + 1) * self.PB
        self.pool = self.buf[x8.LARGE_BASE:x8.LARGE_BASE + self.P * self.PB].view(self.P, PAGE, x8.ROW)
        assert self.pool.is_contiguous() and self.pool.data_ptr() % 32 == 16 and self.pool.numel() > 2 ** 33

    def page(self, n):
        assert 0 <= n < self.P
        return self.buf[x8.LARGE_BASE + n * self.PB:x8.LARGE_BASE + (n + 1) * self.PB]

    def poison(self, pages):
        for n in pages:
            self.page(n).fill_(x8.LARGE_POISON_BYTE)

    def still_poison(self, pages):
        return bool((self.read(pages) == x8.LARGE_POISON_BYTE).all())


@pytest.mark.parametrize("name", ["small-Hi33-T3-p16", "long-Hi33-T1-p16"])
def test_logits_keep_every_bit_when_the_pages_move_past_two_to_the_32(built, dev, buffer, name):
    q, w, (pool, bt), lens, ld = x8.parity_case(name)
    ref, bound, vis = x8.reference(name)
    what = "logits large pool: %s" % name
    pd = pool.to(DEV)
    base = g8.run_logits(q, w, pd, bt, lens, ld)
    g8.check_logits(base, ref, bound, vis, what + ", small pool")
    big = IndexFp8Large(buffer)
    live = ae.live_entries(bt, lens, PAGE)
    plan = x8.large_plan(len(live), seed=len(live))
    assert plan["P"] == big.P
    bt2, pairs, got = lp.relocate(big, pd, bt, lens, plan, first=live[:len(plan["must"])])
    assert got == set(plan["must"])
    moved = g8.run_logits(q, w, big.pool, bt2, lens, ld)
    lp.report(what, big, plan, [n for _, n in pairs])
    g8.check_logits(moved, ref, bound, vis, what + ", large pool")  # finite and within the bound at every visible position
    assert torch.equal(g8.ibits(moved), g8.ibits(base)), what
    assert big.still_poison(plan["poison"] + [plan["dead"]])


@pytest.mark.parametrize("pow2", [False, True], ids=["plain", "pow2"])
def test_append_writes_the_named_pages_and_nothing_else(built, dev, buffer, pow2):
    """The ragged problem at page 16: 0, 1, 5 and 40 new rows, the last two across page edges. The seven pages that receive rows are P - 1
    and the three pages around each of bytes 2^31 and 2^32."""
    p = x8.append_problem("ragged", PAGE)
    bt, lens, cu, k_new = p["bt"], p["lens"], p["cu"], p["k_new"]
    start = torch.full((p["P"], PAGE, x8.ROW), x8.LARGE_POISON_BYTE, dtype=U8)
    args = (k_new.to(DEV), lp.i32(lens), lp.i32(cu))

    def append(pool, table):
        g8.pkg().kv_append_paged_index_bf16_fp8(args[0], pool, table, args[1], args[2], pow2)
        torch.cuda.synchronize()

    small = start.to(DEV)
    append(small, bt.to(DEV))
    assert torch.equal(small.cpu(), x8.append_ref(start, bt, lens, cu, k_new, pow2))
    big = IndexFp8Large(buffer)
    live = ae.live_entries(bt, lens, PAGE)
    recv = lp.receivers(lens, p["new"])
    plan = x8.large_plan(len(live), seed=3)
    assert len(recv) == len(plan["must"]) == 7 and all(e in live for e in recv)
    big.poison(plan["named"])
    bt2, pairs, got = lp.relocate(big, start.to(DEV), bt, lens, plan, first=recv)  # copies poisoned pages
    append(big.pool, bt2)
    after = small.view(-1, big.PB).cpu()
    before = start.view(-1, big.PB)
    written = {n for (j, n) in pairs if not torch.equal(after[j], before[j])}
    assert written == got == set(plan["must"]), (sorted(written), plan["must"])
    assert torch.equal(big.read([n for _, n in pairs]), after[[j for j, _ in pairs]])
    assert big.still_poison(plan["poison"])
    lp.report("fp8 index append large pool: rows written to pages %s" % sorted(written), big, plan, sorted(written))
