"""GPU: the row offset (size_t)tok * (size_t)ld of the DSA indexer in the writer of mla_index_logits_paged_bf16 and in the reader
of mla_index_topk, on a logits tensor of more than 2^32 elements. The largest logits tensor elsewhere is 5 x 5008.

One torch.empty fp32 buffer of 5 (2^30 + 1) elements with 16 guard elements at each end (about 20 GiB) is viewed as [5, 1, ld],
ld = 2^30 + 1: row r starts at element r 2^30 + r -- row 1 just past byte 2^32, row 2 just past element 2^31, row 4 just past element 2^32.
Sequence 0 has length 0, and a 32-bit byte offset (mod 2^30 elements) or element offset (mod 2^32) of any row lands in the first Nmax + 8
elements of row 0: no live row is the wrap image of another (asserted below and in tests/test_mla_index_surface.py). The buffer is never
filled: only the windows [start_r - 8, start_r + Nmax + 8) of the rows and the guard elements are written and read.

The writer: Hi = 17, pages of 16, Nmax = 2048 (two chunks of 1024 keys), lengths [0, 2048, 300, 17, 2000]. The logits of rows 1 ... 4 are
bit-equal to the same problem written with ld = 2048 into a small tensor (which check_logits holds to the fp64 reference); every other
element of every window, the whole window of row 0 included, keeps the sentinel. The reader: NaN in row 0's window, random rows with ties
in rows 1 ... 4 whose true lists are not [0 ... 63], topk = 64: torch.equal with topk_ref on the small rows.

Skipped only on a device with less than 40 GiB in all; a failed allocation is an error.

Not covered: `indices` past 2^31 elements -- it needs topk >= 2^29, which no caller asks for -- and B T near 2^31."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mla_index_reference as ix  # noqa: E402
import test_gpu_mla_index as gi  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
MIN_TOTAL_MEMORY = 40 << 30
LD, NMAX, ROWS, GUARD, MARGIN = ix.ROWS_LD, ix.ROWS_NMAX, len(ix.ROWS_LENS), 16, 8


@pytest.fixture(scope="module")
def rows(built, dev):
    total = torch.cuda.get_device_properties(dev).total_memory
    print("total device memory: %d bytes" % total)
    if total < MIN_TOTAL_MEMORY:
        pytest.skip("a device of %d bytes in all cannot hold a logits tensor of 20 GiB" % total)
    bufs = [torch.empty(ROWS * LD + 2 * GUARD, dtype=torch.float32, device=dev)]  # a failed allocation is an error
    yield bufs
    bufs.clear()
    torch.cuda.empty_cache()


def view(bufs):
    lg = bufs[0][GUARD:GUARD + ROWS * LD].view(ROWS, 1, LD)
    assert lg.is_contiguous() and lg.numel() > 2 ** 32 and lg.data_ptr() == bufs[0].data_ptr() + 4 * GUARD
    return lg


def window(bufs, r):
    """Elements [start_r - 8, start_r + Nmax + 8) of row r, as int32 bits."""
    a = GUARD + r * LD - MARGIN
    return bufs[0][a:a + NMAX + 2 * MARGIN].view(torch.int32)


def ends(bufs):
    return bufs[0][:GUARD].view(torch.int32), bufs[0][GUARD + ROWS * LD:].view(torch.int32)


def test_the_rows_cross_the_boundaries_and_wrap_into_the_empty_row(rows):
    assert ix.ROWS_LENS[0] == 0 and LD == 2 ** 30 + 1
    assert 4 * 1 * LD > 2 ** 32 > 4 * (1 * LD - 8) and 2 * LD > 2 ** 31 > 2 * LD - 8 and 4 * LD > 2 ** 32 > 4 * LD - 8
    for r in range(1, ROWS):
        for image in ix.row_start_wraps(r):
            assert image == r * LD or 0 <= image <= MARGIN, (r, image)  # row 0's window covers [-8, Nmax + 8)
        assert ix.row_start_wraps(r)[0] == r
    assert ix.row_start_wraps(4)[1] == 4
    lg = view(rows)
    assert all(lg[r].data_ptr() - lg.data_ptr() == 4 * r * LD for r in range(ROWS))


def test_logits_writer_reaches_rows_past_two_to_the_32_elements(built, dev, rows):
    q, w, (pool, bt), lens, _ = ix.rows_case()
    ref, bound, vis = ix.logits_ref(q, w, pool, bt, lens, NMAX)
    small = gi.run_logits(q, w, pool, bt, lens, NMAX)
    gi.check_logits(small, ref, bound, vis, "logits large rows: small tensor")
    lg = view(rows)
    for r in range(ROWS):
        window(rows, r).fill_(gi.SENT)
    for e in ends(rows):
        e.fill_(gi.SENT)
    gi.pkg().mla_index_logits_paged_bf16(q.to(DEV), w.to(DEV), pool.to(DEV), bt.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), lg)
    torch.cuda.synchronize()
    pad = torch.full((MARGIN,), gi.SENT, dtype=torch.int32)
    for r in range(ROWS):
        want = torch.cat([pad, gi.ibits(small[r, 0]), pad])
        got = window(rows, r).cpu()
        assert torch.equal(got, want), (r, int((got != want).sum()))
        n = max(vis[r][0], 0)
        assert bool(torch.isfinite(got[MARGIN:MARGIN + n].view(torch.float32)).all())
    assert bool((window(rows, 0).cpu() == gi.SENT).all())
    assert all(bool((e.cpu() == gi.SENT).all()) for e in ends(rows))
    print("logits large rows: last element written at offset %d of %d" % (4 * LD + lens[4] - 1, lg.numel()))


def test_topk_reader_reaches_rows_past_two_to_the_32_elements(built, dev, rows):
    topk = 64
    x, lens = ix.rows_topk_case(topk)
    want = ix.topk_ref(x, lens, topk)
    for b, n in enumerate(lens):  # reading the NaN window of row 0 instead would give another list
        assert n <= topk or want[b, 0].tolist() != list(range(topk))
    lg = view(rows)
    for r in range(ROWS):
        window(rows, r).view(torch.float32).fill_(ix.NAN)
    for r in range(1, ROWS):
        lg[r, 0, :NMAX].copy_(x[r, 0])
    big = torch.full(((ROWS + 2) * topk,), gi.ISENT, dtype=torch.int32, device=DEV)
    idx = big[topk:(ROWS + 1) * topk].view(ROWS, 1, topk)
    gi.pkg().mla_index_topk(lg, torch.tensor(lens, dtype=torch.int32, device=DEV), topk, idx)
    torch.cuda.synchronize()
    flat = big.cpu()
    assert bool((flat[:topk] == gi.ISENT).all()) and bool((flat[(ROWS + 1) * topk:] == gi.ISENT).all()), "guard bands of indices"
    assert torch.equal(idx.cpu(), want), [(b, int((idx.cpu()[b] != want[b]).sum())) for b in range(ROWS)]
