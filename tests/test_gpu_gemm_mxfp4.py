"""GPU: the MXFP4-weight GEMMs and their MXFP8 quantiser (csrc/gemm_mxfp4*.{cuh,hip}, csrc/quant_mxfp8_bf16.*; DESIGN 4.4.32 has the largest
err / bound seen) against tests/gemm_mxfp4_reference.py: the one-hot case that pins nibble order, lanes and scale bytes, exact answers with
guard bands, fp64 under the derived bound, the grouped entry against the dense one per expert, the quantiser's bits, one captured graph."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_mxfp4_reference as mr  # noqa: E402
pytestmark = pytest.mark.gpu

BF, F8, E8 = mr.BF, mr.F8, mr.E8
FILL = 0x7FC1  # a bf16 NaN pattern no kernel writes
FORMS = ("skinny", "tile")


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.uint8)


def gemm(a, sa, b, sb, bias=None, form=None, guard=0):
    """The whole sentinel-filled tensor [guard + M + guard, N] whose middle rows were `out`, copied back."""
    M, N = a.shape[0], b.shape[0]
    whole = torch.full((guard + M + guard, N), FILL, dtype=torch.int16, device="cuda").view(BF)
    pkg().gemm_mxfp4_bf16(a.cuda(), sa.cuda(), b.cuda(), sb.cuda(), whole[guard:guard + M], None if bias is None else bias.cuda(), form)
    torch.cuda.synchronize()
    return whole.cpu()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("step,off", [(8, 3), (37, 5)])
@pytest.mark.parametrize("side", ["a", "b"])
def test_one_hot_rows_pick_single_elements_under_distinct_scales(built, dev, side, step, off, form):
    a, sa, b, sb, want = mr.one_hot(side, step, off)
    assert torch.equal(bits(gemm(a, sa, b, sb, form=form)), bits(want))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M,N,K", mr.SHAPES)
def test_integer_codes_power_of_two_scales_and_bias_are_exact_inside_guard_rows(built, dev, M, N, K, form):
    a, sa, b, sb, bias, want = mr.exact(M, N, K)
    whole = bits(gemm(a, sa, b, sb, bias, form, guard=2))
    assert torch.equal(whole[2:2 + M], bits(want)) and bool((whole[:2] == FILL).all()) and bool((whole[2 + M:] == FILL).all())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M,N,K", [(17, 264, 96), (65, 136, 416), (129, 392, 416), (33, 136, 2880)])
def test_against_fp64_under_the_derived_bound(built, dev, M, N, K, form):
    _, a, sa, b, sb, _, (ref, S) = mr.gaussian(M, N, K)
    out = gemm(a, sa, b, sb, form=form).double()
    ratio = float(((out - ref).abs() / mr.bound(ref, S, K)).max())
    print("gemm_mxfp4 (%d, %d, %d) %s: largest err / bound %.3f" % (M, N, K, form, ratio))
    assert bool(torch.isfinite(out).all()) and ratio <= 1.0, ratio


E, M_TOTAL, GN, GK = 5, 300, 136, 416
# an empty first and an empty middle expert, a 1-row and a 130-row group, starts off the 128-row grid, rows of no expert at both ends
OFFSETS = ((3, 3, 4, 134, 134, 290), (0, 100, 100, 101, 260, 300))


@pytest.mark.parametrize("form", FORMS)
def test_grouped_rows_carry_the_bits_of_the_dense_entry_and_nothing_is_cached(built, dev, form):
    _, a, sa, _, _, _, _ = mr.gaussian(M_TOTAL, GN, GK)
    w = [mr.gaussian(8, GN, GK, seed=e + 1) for e in range(E)]
    b, sb, bias = (torch.stack([c[i] for c in w]) for i in (3, 4, 5))
    ad, sad, bd, sbd, biasd = (t.cuda() for t in (a, sa, b, sb, bias))
    out = torch.empty(M_TOTAL, GN, dtype=BF, device="cuda")
    for offs in OFFSETS:  # the same buffers, other offsets: nothing may be remembered on the host
        out.view(torch.int16).fill_(FILL)
        pkg().gemm_mxfp4_grouped_bf16(ad, sad, bd, sbd, torch.tensor(offs, dtype=torch.int32).cuda(), out, biasd, form)
        got, owned = bits(out.cpu()), torch.zeros(M_TOTAL, dtype=torch.bool)
        for e in range(E):
            r0, r1 = offs[e], offs[e + 1]
            owned[r0:r1] = True
            if r1 > r0:
                assert torch.equal(got[r0:r1], bits(gemm(a[r0:r1], sa[r0:r1], b[e], sb[e], bias[e]))), (offs, e)
        assert bool((got[~owned] == FILL).all())


def quant(x):
    M, K = x.shape
    codes = torch.full((M, K), 0x7F, dtype=torch.uint8, device="cuda").view(F8)
    scales = torch.full((M, K // 32), 0xFF, dtype=torch.uint8, device="cuda").view(E8)
    pkg().quant_mxfp8_bf16(x.cuda(), codes, scales)
    return codes, scales


@pytest.mark.parametrize("M,K", [(3, 96), (130, 416)])
def test_quantiser_equals_the_integer_and_fp32_rule_bit_for_bit(built, dev, M, K):
    x = mr.quant_rows(M, K)
    want_c, want_s = mr.quant_a(x)
    wc, ws = bits(want_c), bits(want_s)
    # the reference alone produces the four situations: a zero block, amax 2^6 -> 2^8, 500 saturating to 448, a subnormal amax under byte 0
    assert int(ws[0, 0]) == 0 and not bool(wc[0, :32].any()) and int(ws[0, 1]) == 125 and int(wc[0, 40]) == 0xF8
    assert int(ws[0, 2]) == 127 and int(wc[0, 70]) == 0x7E and int(ws[-1, 0]) == 0 and int(wc[-1, 3]) == 0x20 and int(wc[-1, 4]) == 0x98
    codes, scales = quant(x)
    assert torch.equal(bits(scales.cpu()), ws) and torch.equal(bits(codes.cpu()), wc)


def test_one_captured_graph_of_quant_and_grouped_gemm_replays_the_eager_bits(built, dev):
    c = pkg()
    xs = [mr.gaussian(M_TOTAL, GN, GK, seed=s)[0] for s in (0, 9)]
    w = [mr.gaussian(8, GN, GK, seed=e + 1) for e in range(E)]
    bd, sbd, biasd = (torch.stack([t[i] for t in w]).cuda() for i in (3, 4, 5))
    off, x = torch.tensor(OFFSETS[0], dtype=torch.int32).cuda(), xs[0].cuda()
    codes, scales = torch.empty(M_TOTAL, GK, dtype=F8, device="cuda"), torch.empty(M_TOTAL, GK // 32, dtype=torch.uint8, device="cuda").view(E8)
    out = torch.empty(M_TOTAL, GN, dtype=BF, device="cuda")

    def step():
        c.quant_mxfp8_bf16(x, codes, scales)
        c.gemm_mxfp4_grouped_bf16(codes, scales, bd, sbd, off, out, biasd)
    eager = []
    for xi in xs:
        x.copy_(xi)
        out.view(torch.int16).fill_(FILL)
        step()
        eager.append(out.cpu())
    assert not torch.equal(bits(eager[0]), bits(eager[1]))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()  # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for i in (0, 1, 0, 1):
        x.copy_(xs[i])
        out.view(torch.int16).fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out.cpu()), bits(eager[i])), i
