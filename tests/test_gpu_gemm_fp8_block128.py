"""GPU: the block-scaled FP8 GEMM and its quantiser (csrc/gemm_fp8_block128.*, csrc/quant_fp8_block128_bf16.*; DESIGN 4.4.27 has the largest
err / bound seen per shape) against tests/gemm_fp8_block128_reference.py: fp64 under the derived bound, exact integer answers, the one-hot case
that pins the operand fragments, guard bands, the quantiser's bits, the quant -> gemm chain and one captured graph."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fp8_block128_reference as gr  # noqa: E402
pytestmark = pytest.mark.gpu

BF, F8, F32 = gr.BF, gr.F8, gr.F32
FILL = 0x7FC1  # a bf16 NaN pattern no kernel writes


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.uint8 if t.dtype == F8 else torch.int32)


def gemm(a, sa, b, sb, front=0, back=0):
    """The whole sentinel-filled tensor [front + M + back, N] whose middle rows were `out`, copied back."""
    M, N = a.shape[0], b.shape[0]
    whole = torch.full((front + M + back, N), FILL, dtype=torch.int16, device="cuda").view(BF)
    pkg().gemm_fp8_block128_bf16(a.cuda(), sa.cuda(), b.cuda(), sb.cuda(), whole[front:front + M])
    torch.cuda.synchronize()
    return whole.cpu()


@pytest.mark.parametrize("M,N,K", gr.SHAPES)
def test_against_fp64_under_the_derived_bound(built, dev, M, N, K):
    _, a, sa, b, sb, (ref, S) = gr.gaussian(M, N, K)
    out = gemm(a, sa, b, sb).double()
    ratio = float(((out - ref).abs() / gr.bound(ref, S, K)).max())
    print("gemm_fp8_block128 (%d, %d, %d): largest err / bound %.3f" % (M, N, K, ratio))
    assert bool(torch.isfinite(out).all()) and ratio <= 1.0, ratio


@pytest.mark.parametrize("M,N,K", gr.SHAPES)
def test_integer_codes_and_power_of_two_scales_are_exact(built, dev, M, N, K):
    a, sa, b, sb, want = gr.exact(M, N, K)
    assert torch.equal(bits(gemm(a, sa, b, sb)), bits(want))


@pytest.mark.parametrize("step,off", [(8, 3), (37, 5)])
@pytest.mark.parametrize("side", ["a", "b"])
def test_one_hot_rows_pick_single_bytes(built, dev, side, step, off):
    a, sa, b, sb, want = gr.one_hot(side, step, off)
    assert torch.equal(bits(gemm(a, sa, b, sb)), bits(want))


@pytest.mark.parametrize("M,N,K", [(17, 264, 384), (129, 392, 1024)])
def test_rows_in_front_of_and_behind_out_keep_their_bits(built, dev, M, N, K):
    a, sa, b, sb, want = gr.exact(M, N, K)
    whole = bits(gemm(a, sa, b, sb, front=3, back=2))
    assert torch.equal(whole[3:3 + M], bits(want)) and bool((whole[:3] == FILL).all()) and bool((whole[3 + M:] == FILL).all())


def quant(x, pow2):
    M, K = x.shape
    codes = torch.full((M, K), 0x7F, dtype=torch.uint8, device="cuda").view(F8)
    scales = torch.full((M, K // 128), float("nan"), dtype=F32, device="cuda")
    pkg().quant_fp8_block128_bf16(x.cuda(), codes, scales, scale_pow2=pow2)
    return codes, scales


@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("M,K", [(1, 128), (65, 384), (3, 7168)])
def test_quantiser_equals_the_fp32_formula_bit_for_bit(built, dev, M, K, pow2):
    g = torch.Generator().manual_seed(M + K)
    x = (torch.randn(M, K, generator=g) * 2.0 ** (torch.rand(M, 1, generator=g) * 8 - 4)).to(BF)
    x[M // 2] = 0                                  # an all-zero row: scale = 1e-4 / 448, codes 0
    x[-1, :128] = x[-1, :128].clamp(-50, 50)
    x[-1, 5], x[-1, 77] = 56.0, -56.0              # a block whose amax is 448 * 2^-3: the codes +-448
    codes, scales = quant(x, pow2)
    want_c, want_s = gr.quant_a(x, pow2)
    assert torch.equal(bits(scales.cpu()), bits(want_s)) and torch.equal(bits(codes.cpu()), bits(want_c))
    assert {int(v) for v in bits(codes.cpu())[-1, [5, 77]]} == {0x7E, 0xFE}


@pytest.mark.parametrize("M,N,K", [(17, 264, 384), (129, 392, 1024)])
def test_quant_then_gemm_equals_gemm_on_the_helpers_codes(built, dev, M, N, K):
    x, a, sa, b, sb, _ = gr.gaussian(M, N, K)
    codes, scales = quant(x, False)
    out = torch.empty(M, N, dtype=BF, device="cuda")
    pkg().gemm_fp8_block128_bf16(codes, scales, b.cuda(), sb.cuda(), out)
    assert torch.equal(bits(out.cpu()), bits(gemm(a, sa, b, sb)))


def test_one_captured_graph_of_quant_and_gemm_replays_on_a_second_input(built, dev):
    M, N, K = 17, 264, 384
    c, (x0, _, _, b, sb, _), x1 = pkg(), gr.gaussian(M, N, K), gr.gaussian(64, 128, K)[0][:M]
    bd, sbd, x = b.cuda(), sb.cuda(), x0.cuda()
    codes, scales, out = torch.empty(M, K, dtype=F8, device="cuda"), torch.empty(M, K // 128, dtype=F32, device="cuda"), torch.empty(M, N, dtype=BF, device="cuda")

    def step():
        c.quant_fp8_block128_bf16(x, codes, scales)
        c.gemm_fp8_block128_bf16(codes, scales, bd, sbd, out)
    eager = []
    for xi in (x0, x1):
        x.copy_(xi)
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
        x.copy_((x0, x1)[i])
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out.cpu()), bits(eager[i])), i
