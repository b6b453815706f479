"""CPU only: the case table of tests/fa_plain_cases.py, proven before tests/test_gpu_fa2_plain_edges.py and
tests/test_gpu_fa2_plain_large.py run it. (1) Every row reaches the kernel it is listed under, by the text of manifest.describe (the plan
of fa2_plan, csrc/flash_attn.hip) at stages 1 and 2, and the table keeps every kind, every head dim and for every kind a head count that is
and one that is not a multiple of 8. (2) The one-hot problem of every (N, D) of the table meets its conditions: a gap of >= 20 nats, a key
code over >= 85 % of D (at D = 32: 30 of 32 dimensions, 28 at N = 128, whose 7 code bits fit 4 times), an off-target mass <= 2.3e-8, and
the fp64 softmax inside the bound 2^-10 |V[pi]| + 1e-5 of the GPU test with 9e-6 to spare. (3) Every case past 2^32 bytes does cross that line by 8 heads, fits the grid,
and its period of 7 heads separates every image of a 32-bit wrap: a wrapped access lands on a head with another residue."""
import pytest

import fa_plain_cases as fc


@pytest.mark.parametrize("row", fc.TABLE + fc.LONG + fc.LARGE, ids=fc.row_id)
def test_every_row_reaches_the_kernel_it_is_listed_under(built, row):
    kind, name, B, H, N, D = row
    two, one = (built.manifest.describe(name, (B, H, N, D), st) for st in (2, 1))
    assert fc.reaches(two, row) and fc.reaches(one, row), (row, two, one)
    if kind != "splitkv":  # (the split-KV rung names its two forms in the text itself)
        assert one.replace("load-then-compute", "prefetch") == two + " [single stage: every tile fetch waited for where it is issued]", (one, two)


def test_table_keeps_every_kind_head_dim_and_both_head_maps():
    assert len(set(fc.TABLE)) == len(fc.TABLE)
    assert {r[0] for r in fc.TABLE} == set(fc.KINDS)
    assert {r[5] for r in fc.TABLE} == set(fc.HEAD_DIMS)
    for kind in fc.KINDS:
        counts = [r[2] * r[3] for r in fc.TABLE if r[0] == kind]
        # n_heads % 8 == 0: heads pinned to the XCDs; otherwise the plain block-id -> head map
        assert any(n % 8 == 0 for n in counts) and any(n % 8 != 0 for n in counts), (kind, counts)
    for kind, vt in (("v2/2", True), ("v2/4", True), ("m16x", True), ("m16x64r", True)):
        assert any(r[0] == kind and r[1] == fc.VT for r in fc.TABLE), kind
    assert {r[0] for r in fc.LARGE} == {"dw4", "pair2", "m16x64r", "m16x", "v2/8"}


@pytest.mark.parametrize("N,D", sorted({(r[4], r[5]) for r in fc.TABLE}))
def test_onehot_problem_meets_its_conditions(N, D):
    gap, span, mass, over, target = fc.onehot_facts(N, D, seed=11 * N + D)
    print("onehot N=%d D=%d: gap %.1f nats, code over %d of %d dimensions, off-target mass %.2e, fp64 O - bound %.2e, target %.0f nats"
          % (N, D, gap, span, D, mass, over, target))
    assert gap >= 20.0 - 1e-9
    assert span >= 0.85 * D and (D != 32 or span >= (28 if N == 128 else 30))  # 7 code bits x 4 at N = 128: 28 of 32; every other N at D = 32: >= 30
    assert mass <= 2.3e-8
    assert over <= -9e-6  # the fp64 softmax uses less than a tenth of the additive term: the rest is the kernel's


@pytest.mark.parametrize("row", fc.LARGE, ids=fc.row_id)
def test_large_cases_cross_4_gib_and_separate_every_wrap_image(row):
    kind, name, B, H, N, D = row
    assert B == 1 and B * H * (N // 32 + 1) <= 2 ** 31 - 1
    line = 2 ** 32 // (2 * N * D)  # the first head that lies wholly beyond byte 2^32
    assert line * 2 * N * D == 2 ** 32 and H >= line + 8 and H * N * D * 2 > 2 ** 32
    assert H > fc.PERIOD
    for what, shift in fc.wrap_shifts(N, D).items():
        assert shift >= 1 and shift & (shift - 1) == 0 and shift % fc.PERIOD != 0, (what, shift)
        images = [(h, h - shift) for h in range(shift, H)]  # the heads a wrapped access of head h would touch instead
        if what != "2^32 elements":
            assert len(images) >= 8, (what, shift)  # this wrap does happen inside the tensor
        assert all(h % fc.PERIOD != i % fc.PERIOD for h, i in images), what
