"""GPU: multi-token decode attention (T <= 8) over a paged KV cache held in FP8 (cuda_learn_notes_amd.fa2_decode_paged_multi_fp8,
cln_fa2_decode_paged_multi_fp8; csrc/flash_attn_decode_paged_multi_fp8.cuh) against the fp64 reference of tests/fp8_paged_attn_reference.py ON
THE DEQUANTISED POOLS, with the bounds decode_reference.fa_tol / lse_tol unchanged: the codes are exact in fp16 and the scales enter in fp32, so
the kernel's error is that of the fp16 kernel. What quantising the cache costs is printed, not asserted. The shapes, MIXED and the boundary
lengths are those of tests/test_gpu_fa2_decode_paged_multi.py (the plan is the same); the cases are those of tests/fp8_paged_attn_cases.py, which
the prefill entry shares. Every case prints its figures before it asserts (pytest -s)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_paged_attn_cases as cs  # noqa: E402
import fp8_paged_attn_reference as fr  # noqa: E402
import test_gpu_fa2_decode_paged_multi as base  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES, MIXED, DS, ids = base.SHAPES, base.MIXED, base.DS, base.ids
E = cs.Entry("multi")


def plan_of(shape, D):
    B, Hkv, G, page, mp, T = shape
    return fr.plan(B, T, Hkv * G, Hkv, mp, page, D)


def test_shapes_cover_the_plan(built):
    for D in DS:
        splits = [built.fa2_decode_paged_multi_fp8_plan(B, T, Hkv * G, Hkv, mp, page, D)[0] for (B, Hkv, G, page, mp, T) in SHAPES]
        assert splits == [plan_of(s, D)[0] for s in SHAPES]
        assert any(s == 1 for s in splits) and any(s >= 3 for s in splits), (D, splits)
        for s in SHAPES + [MIXED]:  # the boundary lengths of the fp16 file are built on the same plan
            assert plan_of(s, D) == base.plan_of(s, D)
    assert any(s[3] < fr.KEY_STEP for s in SHAPES) and any(s[3] > fr.KEY_STEP for s in SHAPES)
    assert max(s[3] * s[4] for s in SHAPES + [MIXED]) <= 8192
    assert plan_of(MIXED, 64)[0] >= 3


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parity_at_the_plan_and_mask_boundaries(built, dev, shape, D):
    cs.parity(E, shape, D, base.lengths_for(shape, D))


@pytest.mark.parametrize("D", DS)
def test_mixed_batch_empty_sequence_and_clamped_lengths(built, dev, D):
    cs.mixed_empty_and_clamped(E, MIXED, D, plan_of(MIXED, D)[1] + 1)  # the second split holds one key, which only the last query sees


@pytest.mark.parametrize("D", DS)
def test_every_code_converts_exactly(built, dev, D):
    cs.every_code_converts_exactly(E, D, 8, 2)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(1, 1, 8, 16, 48, 8), (1, 2, 2, 32, 40, 5), (2, 1, 4, 64, 3, 2)], ids=ids)
def test_causal_tail_is_masked_not_down_weighted(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    S, C, _ = plan_of(shape, D)
    lens = [min(C + T // 2, page * mp), page * mp - 1][:B]  # causal edges across a split boundary where there is one
    cs.causal_tail_is_masked(E, shape, D, lens, list(range(T - 1)))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [MIXED, (1, 2, 2, 32, 40, 5), (2, 1, 4, 64, 3, 2)], ids=ids)
def test_nothing_outside_the_live_rows_is_used(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    S, C, _ = plan_of(shape, D)
    lens = [C + 1, page * mp - 1, 5][:B] if S > 1 else [page + 1, page * mp - 1, 5][:B]
    cs.nothing_outside_the_live_rows(E, shape, D, lens)


@pytest.mark.parametrize("D", DS)
def test_bits_do_not_depend_on_placement_or_neighbours_and_calls_repeat(built, dev, D):
    cs.placement_neighbours_and_repeats(E, MIXED, D, [700, 999, 333])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(1, 2, 2, 32, 40, 5), MIXED, (1, 2, 4, 128, 2, 1), (2, 3, 4, 16, 40, 5)], ids=ids)  # the last: Hkv = 3
def test_scale_algebra_bit_for_bit(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.scale_algebra(E, shape, D, [page * mp - 3, page * mp // 2 + 1, T + 7][:B])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(1, 2, 2, 32, 40, 5), (1, 1, 8, 16, 48, 8)], ids=ids)
def test_agreement_with_the_fp16_entry_on_the_codes(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.agrees_with_the_fp16_entry(E, shape, D, [page * mp - 3])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 1, 4, 32, 32, 1), (1, 2, 4, 128, 2, 1), (2, 2, 8, 16, 64, 1), (1, 1, 1, 16, 63, 1)], ids=ids)
def test_one_token_agrees_with_the_single_query_fp8_entry(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.multi_at_one_token_agrees_with_decode(shape, D, [page * mp - 16, 385, 3][:B] if page * mp >= 401 else [page * mp - 1] * B)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 1, 4, 32, 32, 5), (1, 2, 2, 16, 24, 8)], ids=ids)
def test_agrees_with_the_prefill_entry(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.prefill_agrees_with_multi(shape, D, [page * mp - 16, 385, 3][:B])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [MIXED, (2, 1, 4, 64, 3, 2), (1, 1, 8, 16, 48, 8)], ids=ids)
def test_guard_bands_and_workspaces(built, dev, shape, D):
    B, Hkv, G, page, mp, T = shape
    cs.guard_bands_and_workspaces(E, shape, D, [page * mp, 1, page * mp // 2][:B])


@pytest.mark.parametrize("D", DS)
def test_serving_chain_append_prefill_then_multi_token_steps(built, dev, D):
    cs.serving_chain(D)


@pytest.mark.parametrize("D", DS)
def test_graph_replay_of_append_and_attention_reads_everything_from_the_device(built, dev, D):
    cs.graph_replay(E, D, 3)


def test_python_argument_errors(built, dev):
    cs.python_argument_errors(E, 3)
