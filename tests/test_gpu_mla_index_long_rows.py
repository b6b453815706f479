"""GPU: cuda_learn_notes_amd.mla_index_topk (csrc/mla_index_topk.*) on rows of more than two scan blocks, on topk above the
scan block, and on rows at every 4-byte residue of a 16-byte boundary; mla_index_logits_paged_bf16 writing rows of such strides.

The ordered pass of the kernel keeps its per-wave counts in tot[blk & 1] and carries run_gt / run_eq from block to block of 4096
positions. tests/test_gpu_mla_index.py stops at n = 5000 and topk = 2048: two blocks, every count buffer written once, one carry, a list
that fills inside one block. Here: n = 8191 ... 20481 (2 ... 6 blocks, ragged last blocks) and the production row of 131072 (32 blocks),
topk 1 ... 6000, on the five value recipes of tests/mla_index_reference.long_row. tests/test_mla_index_surface.py proves on the CPU that
every recipe has the property it claims, and that a model of the kernel with a stale count buffer, a lost carry, a pass that ends after two
blocks or the wrong ties differs from the reference on these rows -- and that the first three cannot show on the rows the suite had.

The oracle is torch.equal with ix.topk_ref: no tolerance. NaN poison at every j >= n, guard bands around the lists (run_topk)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mla_index_reference as ix  # noqa: E402
import test_gpu_mla_index as gi  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ix.LONG_KINDS)
@pytest.mark.parametrize("topk", ix.long_topks())
def test_topk_is_exact_on_rows_of_two_to_six_scan_blocks(built, dev, topk, kind):
    """B = 1, ld = 20488, n in {8191, 8192, 8193, 12288, 12289, 16384, 16385, 20481}; a combination the recipe cannot hold (n <= topk;
    straddle at n <= 12288 or topk = 1) is passed over, the others are counted."""
    ran = 0
    for n in ix.long_ns():
        case = ix.long_logits(kind, n, topk)
        if case is None:
            continue
        logits, lens = case
        assert logits.shape == (1, 1, ix.LONG_TOPK_LD) and bool(torch.isnan(logits[0, 0, n:]).all())
        got = gi.run_topk(logits, lens, topk)
        want = ix.topk_ref(logits, lens, topk)
        assert torch.equal(got, want), (kind, topk, n, int((got != want).sum()))
        ran += 1
    print("top-k long rows %s topk=%d: %d rows exact" % (kind, topk, ran))
    assert ran >= (4 if kind == "straddle" else 6) or (kind == "straddle" and topk == 1 and ran == 0)


@pytest.mark.parametrize("kind", ix.LONG_KINDS)
def test_topk_is_exact_on_the_production_row(built, dev, kind):
    """n = ld = 131072: 32 scan blocks, every count buffer used sixteen times; topk = 2048."""
    logits, lens = ix.long_logits(kind, ix.PROD_N, 2048, ld=ix.PROD_N)
    got = gi.run_topk(logits, lens, 2048)
    assert torch.equal(got, ix.topk_ref(logits, lens, 2048)), kind


def test_topk_with_a_negative_length_gives_the_empty_list(built, dev):
    """max(seqlens[b], 0): a sequence of length -5 between two live ones reads nothing and its lists are all -1, for every token."""
    B, T, ld, topk = 3, 2, 300, 64
    logits = (torch.randint(-20, 21, (B, T, ld), generator=torch.Generator().manual_seed(6)).float() / 8).contiguous()
    logits[1] = ix.NAN
    lens = [200, -5, 70]
    got = gi.run_topk(logits, lens, topk)
    assert torch.equal(got, ix.topk_ref(logits, lens, topk)) and bool((got[1] == -1).all()) and int(got[0].min()) >= 0


# ---------------------------------------------------------------------------------------------------- rows at 0, 4, 8, 12 bytes past 16

@pytest.mark.parametrize("shift", [False, True], ids=["base0", "base4"])
@pytest.mark.parametrize("kind", ix.ALIGN_KINDS)
@pytest.mark.parametrize("ld", ix.ALIGN_LDS)
def test_topk_reads_rows_at_every_residue(built, dev, ld, kind, shift):
    """B = 2, T = 3, ld = 4101, 4102, 4103: the six rows of ONE call start at 0, 4, 8 and 12 bytes past a 16-byte boundary (ld = 4102: at 0
    and 8, at 4 and 12 with the tensor itself 4 bytes in) -- read off data_ptr() here. load4's dwordx4 promises 4-byte alignment only. The
    lengths make n = 4097, 4100 and ld occur; topk 64 and 2048."""
    seen = set()
    for which in (0, 1):
        logits, lens = ix.align_case(ld, kind, which)
        for topk in (64, 2048):
            ptrs = []
            got = gi.run_topk(logits, lens, topk, shift=shift, ptrs=ptrs)
            assert torch.equal(got, ix.topk_ref(logits, lens, topk)), (ld, kind, which, topk)
            res = [(ptrs[0] + 4 * r * ld) % 16 for r in range(ix.ALIGN_B * ix.ALIGN_T)]
            assert res == ix.row_residues(ld, base=4 if shift else 0)
            seen |= set(res)
    assert seen == ({0, 4, 8, 12} if ld % 2 else ({4, 12} if shift else {0, 8})), (ld, sorted(seen))


@pytest.mark.parametrize("ld", ix.ALIGN_LDS)
def test_logits_writes_rows_of_odd_strides(built, dev, ld):
    """Hi = 17, T = 3, ld = 4101, 4102, 4103 (ld mod 4 = 1, 2, 3; cap = the cache's 320): within the derived bound, nothing written past vis."""
    q, w, (pool, bt), lens, _ = ix.one_case(17, 3, 16)
    ref, bound, vis = ix.logits_ref(q, w, pool, bt, lens, ld)
    gi.check_logits(gi.run_logits(q, w, pool, bt, lens, ld), ref, bound, vis, "logits odd stride: ld=%d" % ld)


def test_zz_summary_of_error_over_bound(built, dev):
    """The largest logit err / bound of this file's parity cases. Not an assertion of its own -- every case asserted err <= bound."""
    mine = {g: r for g, r in gi.RATIOS.items() if g == "logits odd stride"}
    for group, r in sorted(mine.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert mine and all(r <= 1.0 for r in mine.values())
