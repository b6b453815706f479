"""GPU: the DSA indexer's two entries that address the paged index-key cache -- mla_index_logits_paged_bf16 and kv_append_paged_index_bf16
 -- over a pool of more than 2^32 elements. Both form the pool offset ((pg << page_shift) + row) 128 behind a (size_t) cast
that no other test holds up: the largest index pool elsewhere is a few MiB.

The pool is the bf16 [P, 16, 128] view of the 8 GiB buffer of tests/test_gpu_paged_mla_large_pool.py, 16 bytes in: E = 2048 elements a page,
2 bytes an element, P = 2^21 + 16 pages, so the view ends just past element 2^32 (byte 2^33). E is a power of two, so the plan is
tests/paged_large_pool.plan's (proven for this geometry and these page counts by tests/test_paged_large_pool_plan.py): named pages at P - 1
and on both sides of elements 2^31 and 2^32, NaN poison on every 32-bit wrap image of a named page, on its neighbours and on pages 0 .. 7.

The oracle adds no tolerance. Logits: a case of tests/mla_index_reference.py runs on its small pool and is held to the fp64 reference by
check_logits; its live pages are copied on the device to the named pages, the table is remapped, the dead entries point at a poison page,
and the entry runs again: the logits keep every bit and are finite, the sampled poison pages still hold poison. Every live page is read (the
last token sees the whole sequence), so P - 1 and the pages at and above each boundary are read. Append: both pools start from poison;
afterwards every named page of the large view equals its page of the small pool byte for byte and the poison pages hold poison.

The module is skipped only on a device with less than 16 GiB in all (the imported fixture); a failed allocation is an error."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mla_index_reference as ix  # noqa: E402
import paged_all_entries as ae  # noqa: E402
import paged_large_pool as plp  # noqa: E402
import test_gpu_mla_index as gi  # noqa: E402
import test_gpu_paged_mla_large_pool as lp  # noqa: E402

pytestmark = pytest.mark.gpu

buffer = lp.buffer  # the module-scoped 8 GiB byte buffer, allocated once for this module
BF, DEV, PAGE = torch.bfloat16, "cuda", 16
E, S = PAGE * ix.D, 2


class IndexLarge(lp.Large):
    """The [P, 16, 128] bf16 view of the buffer."""

    def __init__(self, bufs):
        self.dtype, self.s, self.E = BF, S, E
        self.PB, self.P = E * S, plp.pages(E, S)
        self.buf = bufs[0]
        assert self.P == 2 ** 21 + 16 and plp.BASE + self.P * self.PB <= plp.BUF_BYTES == self.buf.numel()
        self.pool = self.buf[plp.BASE:plp.BASE + self.P * self.PB].view(BF).view(self.P, PAGE, ix.D)
        assert self.pool.is_contiguous() and self.pool.data_ptr() % 32 == 16 and 2 ** 32 < self.pool.numel() < 2 ** 32 + 17 * E


def index_plan(big, n_live, seed):
    """paged_large_pool.plan with "must": P - 1, the two pages at and above every boundary and the highest named page below it."""
    plan = plp.plan(E, S, n_live, seed=seed)
    assert plan["P"] == big.P
    must = [big.P - 1]
    for b in plp.boundaries(E, S):
        must += [b, b + 1, max(n for n in plan["named"] if n < b)]
    assert all(n in plan["named"] for n in must) and len(set(must)) == 7
    plan["must"] = must
    return plan


@pytest.mark.parametrize("case", ["one", "long"])
def test_logits_keep_every_bit_when_the_pages_move_past_two_to_the_32(built, dev, buffer, case):
    q, w, (pool, bt), lens, ld = ix.one_case(17, 3, 16) if case == "one" else ix.long_case()
    ref, bound, vis = ix.reference("one", 17, 3, 16) if case == "one" else ix.reference("long")
    what = "logits large pool: %s" % case
    pd = pool.to(DEV)
    base = gi.run_logits(q, w, pd, bt, lens, ld)
    gi.check_logits(base, ref, bound, vis, what + ", small pool")
    big = IndexLarge(buffer)
    live = ae.live_entries(bt, lens, PAGE)
    plan = index_plan(big, len(live), seed=len(live))
    bt2, pairs, got = lp.relocate(big, pd, bt, lens, plan, first=live[:len(plan["must"])])
    assert got == set(plan["must"])
    moved = gi.run_logits(q, w, big.pool, bt2, lens, ld)
    lp.report(what, big, plan, [n for _, n in pairs])
    gi.check_logits(moved, ref, bound, vis, what + ", large pool")  # finite and within the bound at every visible position
    assert torch.equal(gi.ibits(moved), gi.ibits(base)), what
    assert big.still_poison(plan["poison"][:4] + plan["poison"][-4:] + [plan["dead"]])


def test_append_writes_the_named_pages_and_nothing_else(built, dev, buffer):
    """The ragged problem of tests/test_gpu_mla_index.py's append tests: 0, 1, 5 and 40 new rows, the last two across page edges. The seven
    pages that receive rows are P - 1 and three pages around each of 2^31 and 2^32."""
    p = ix.append_problem("ragged")
    bt, lens, cu, k_new = p["bt"], p["lens"], p["cu"], p["k_new"]
    start = ae.poisoned((p["P"], PAGE, ix.D), BF)
    args = (k_new.to(DEV), lp.i32(lens), lp.i32(cu))

    def append(pool, table):
        gi.pkg().kv_append_paged_index_bf16(args[0], pool, table, args[1], args[2])
        torch.cuda.synchronize()

    small = start.to(DEV)
    append(small, bt.to(DEV))
    want = ix.append_ref(start, bt, lens, cu, k_new)
    assert torch.equal(small.cpu().view(torch.int16), want.view(torch.int16))
    big = IndexLarge(buffer)
    live = ae.live_entries(bt, lens, PAGE)
    recv = lp.receivers(lens, p["new"])
    plan = index_plan(big, len(live), seed=3)
    assert len(recv) == len(plan["must"]) == 7 and all(x in live for x in recv)
    big.poison(plan["named"])
    bt2, pairs, got = lp.relocate(big, start.to(DEV), bt, lens, plan, first=recv)  # copies poisoned pages
    append(big.pool, bt2)
    after = small.view(torch.uint8).view(-1, big.PB).cpu()
    before = start.view(torch.uint8).view(-1, big.PB)
    written = {n for (j, n) in pairs if not torch.equal(after[j], before[j])}
    assert written == got == set(plan["must"]), (sorted(written), plan["must"])
    assert torch.equal(big.read([n for _, n in pairs]), after[[j for j, _ in pairs]])
    assert big.still_poison(plan["poison"])
    lp.report("index append large pool: rows written to pages %s" % sorted(written), big, plan, sorted(written))


def test_zz_summary_of_error_over_bound(built, dev):
    """The largest logit err / bound of this file's runs. Not an assertion of its own; the large-pool runs are held by bit equality."""
    mine = {g: r for g, r in gi.RATIOS.items() if g == "logits large pool"}
    for group, r in sorted(mine.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert all(r <= 1.0 for r in mine.values())
