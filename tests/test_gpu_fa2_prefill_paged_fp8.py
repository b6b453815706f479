"""GPU: prefill attention (any T) over a paged KV cache held in FP8 (cuda_learn_notes_amd.fa2_prefill_paged_fp8, cln_fa2_prefill_paged_fp8;
csrc/flash_attn_prefill_paged_fp8.cuh) against the fp64 reference of tests/fp8_paged_attn_reference.py ON THE DEQUANTISED POOLS, with the bounds
decode_reference.fa_tol / lse_tol unchanged: the codes are exact in fp16 and the scales enter in fp32, so the kernel's error is that of the fp16
kernel. What quantising the cache costs is printed, not asserted. The shapes, MIXED and the boundary lengths are those of
tests/test_gpu_fa2_prefill_paged.py; the cases are those of tests/fp8_paged_attn_cases.py, which the multi-token entry shares
(the serving chain, which runs both entries, is in tests/test_gpu_fa2_decode_paged_multi_fp8.py). Every case prints
its figures before it asserts (pytest -s)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_paged_attn_cases as cs  # noqa: E402
import prefill_reference as pf  # noqa: E402
import test_gpu_fa2_prefill_paged as base  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES, MIXED, DS, ids = base.SHAPES, base.MIXED, base.DS, base.ids
E = cs.Entry("prefill")


def test_shapes_are_the_fp16_ones_and_the_tile_is_the_kernels(built):
    assert max(s[3] * s[4] for s in SHAPES + [MIXED]) <= 8192
    for s in SHAPES + [MIXED]:
        B, Hkv, G, page, mp, T = s
        t = built.manifest.describe_prefill_paged_fp8(B, T, Hkv * G, Hkv, mp, page, 128)
        assert " rows=%d keys=%d:" % (base.ROWS, base.STEP) in t and "%d workgroups" % (B * Hkv * pf.tiles(T, G)) in t, t


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parity_at_the_tile_page_and_mask_boundaries(built, dev, shape, D):
    cs.parity(E, shape, D, base.lengths_for(shape))


@pytest.mark.parametrize("D", DS)
def test_mixed_batch_empty_sequence_and_clamped_lengths(built, dev, D):
    cs.mixed_empty_and_clamped(E, MIXED, D, MIXED[5] - 7)  # a mid value whose first queries see nothing


@pytest.mark.parametrize("D", DS)
def test_every_code_converts_exactly(built, dev, D):
    cs.every_code_converts_exactly(E, D, 70, 2)  # R = 140: a whole workgroup tile and a partly empty one


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(1, 1, 8, 16, 20, 17), (2, 2, 4, 64, 8, 33), (1, 2, 1, 32, 40, 130)], ids=ids)
def test_causal_tail_is_masked_not_down_weighted(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    lens = [min(base.STEP + T // 2 + 1, page * mp), page * mp - 3][:B]
    ts = base.edge_tokens(T, G)
    assert 0 in ts and T - 2 in ts and (base.ROWS - 1) // G in ts and base.ROWS // G in ts + [T - 1]
    cs.causal_tail_is_masked(E, shape, D, lens, ts)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [MIXED, (1, 2, 1, 32, 40, 130), (2, 2, 4, 64, 8, 33)], ids=ids)
def test_nothing_outside_the_live_rows_is_used(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.nothing_outside_the_live_rows(E, shape, D, [page + 1, page * mp - 1, 5][:B])


@pytest.mark.parametrize("D", DS)
def test_bits_do_not_depend_on_placement_or_neighbours_and_calls_repeat(built, dev, D):
    cs.placement_neighbours_and_repeats(E, MIXED, D, [700, 999, 333])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 64, 8, 33), MIXED, (1, 3, 2, 16, 12, 70)], ids=ids)  # the last: Hkv = 3, R = 140 rows
def test_scale_algebra_bit_for_bit(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.scale_algebra(E, shape, D, [page * mp - 3, page * mp // 2 + 1, T + 7][:B])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 64, 8, 33), (1, 2, 1, 32, 40, 130)], ids=ids)
def test_agreement_with_the_fp16_entry_on_the_codes(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.agrees_with_the_fp16_entry(E, shape, D, [page * mp - 3, page * mp // 2 + 1][:B])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 1, 4, 32, 32, 1), (3, 1, 4, 32, 32, 5), (1, 2, 2, 16, 24, 8), (1, 1, 8, 128, 4, 8)], ids=ids)
def test_few_tokens_agree_with_the_multi_token_entry(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.prefill_agrees_with_multi(shape, D, [page * mp - 16, 385, 3][:B])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [MIXED, (1, 1, 8, 16, 20, 17)], ids=ids)
def test_guard_bands(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.guard_bands_and_workspaces(E, shape, D, [page * mp, 1, page * mp // 2][:B])


@pytest.mark.parametrize("D", DS)
def test_graph_replay_of_append_and_prefill_reads_everything_from_the_device(built, dev, D):
    cs.graph_replay(E, D, 40)


def test_python_argument_errors(built, dev):
    cs.python_argument_errors(E, 40)
