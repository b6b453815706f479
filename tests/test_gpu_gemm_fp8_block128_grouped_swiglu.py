"""GPU: the fused gate/up + SiLU-mul + quantise grouped FP8 GEMM (csrc/gemm_fp8_block128_grouped_swiglu.*; DESIGN 4.4.30 has the largest
err / bound seen per case) against tests/gemm_fp8_block128_swiglu_reference.py, per expert: fp64 under the derived bound, bit-equal codes
and scales on integer inputs with every guard row and row of no expert untouched, and one captured graph over two offset arrays. The case
set is the grouped tests' (E = 7, sizes (0, 1, 17, 65, 130, 0, 64), 3 trailing rows of no expert) at I = 256: two column blocks, so the up
half's scale-block index I / 128 + t differs from t."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fp8_block128_reference as gr  # noqa: E402
import gemm_fp8_block128_swiglu_reference as sr  # noqa: E402
from test_gpu_gemm_fp8_block128 import bits, pkg  # noqa: E402
from test_gpu_gemm_fp8_block128_grouped import FORMS, GUARD, SIZES, TRAIL, groups, offsets  # noqa: E402
pytestmark = pytest.mark.gpu

I, KS = 256, (384, 1024)  # K / 128 = 3 below the four-block ring; the ring wrapping twice
CODE_FILL, SCALE_FILL = 0x7F, 0x7FC00001  # the e4m3fn NaN code and an fp32 NaN pattern no kernel writes


@functools.lru_cache(maxsize=None)
def gaussian(K):
    """a, sa of sum(SIZES) + TRAIL Gaussian rows, per expert its own quantised 0.05 randn gate | up weight, and per non-empty expert
    (h_ref, E_h) in fp64."""
    g = torch.Generator().manual_seed(1013 * I + K)
    a, sa = gr.quant_a(torch.randn(sum(SIZES) + TRAIL, K, generator=g).to(gr.BF))
    b, sb = zip(*(gr.quant_b(0.05 * torch.randn(2 * I, K, generator=g)) for _ in SIZES))
    refs = {e: sr.ref(a[r0:r1], sa[r0:r1], b[e], sb[e], K) for e, r0, r1 in groups(SIZES)}
    return a, sa, torch.stack(b), torch.stack(sb), refs


@functools.lru_cache(maxsize=None)
def exact(K):
    """sr.exact per expert (an empty expert and the trailing rows get a case of their own that no answer may show), and per non-empty expert
    the fp32 product hf."""
    cases = [sr.exact(m if m else 5 + e, I, K) for e, m in enumerate(SIZES)] + [sr.exact(TRAIL, I, K)]
    rows = [c for c, m in zip(cases, SIZES + (TRAIL,)) if m]
    want = {e: cases[e][4] for e, _, _ in groups(SIZES)}
    return (torch.cat([c[0] for c in rows]), torch.cat([c[1] for c in rows]), torch.stack([c[2] for c in cases[:-1]]),
            torch.stack([c[3] for c in cases[:-1]]), want)


def fused(a, sa, b, sb, off, form, pow2=False):
    """The whole sentinel-filled h [GUARD + M_total + GUARD, I] (bytes) and h_scale [.., I / 128] (int32 bits), copied back."""
    M = a.shape[0]
    h = torch.full((GUARD + M + GUARD, I), CODE_FILL, dtype=torch.uint8, device="cuda")
    hs = torch.full((GUARD + M + GUARD, I // 128), SCALE_FILL, dtype=torch.int32, device="cuda")
    pkg().gemm_fp8_block128_grouped_swiglu_fp8(a.cuda(), sa.cuda(), b.cuda(), sb.cuda(), off.cuda(), h[GUARD:GUARD + M].view(gr.F8),
                                               hs[GUARD:GUARD + M].view(torch.float32), form=form, scale_pow2=pow2)
    torch.cuda.synchronize()
    return h.cpu(), hs.cpu()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", KS)
def test_each_expert_against_fp64_under_the_derived_bound(built, dev, K, form):
    a, sa, b, sb, refs = gaussian(K)
    h, hs = fused(a, sa, b, sb, offsets(SIZES), form)
    h, hs = h[GUARD:-GUARD].view(gr.F8).double(), hs[GUARD:-GUARD].view(torch.float32)
    ratio = scale_ratio = 0.0
    for e, r0, r1 in groups(SIZES):
        ref, Eh = refs[e]
        got = h[r0:r1] * hs[r0:r1].double().repeat_interleave(128, dim=1)
        ratio = max(ratio, float(((got - ref).abs() / sr.bound(ref, Eh, hs[r0:r1])).max()))
        err, allowed = sr.scale_slack(ref, Eh, hs[r0:r1])
        scale_ratio = max(scale_ratio, float((err / allowed).max()))
    print("gemm_fp8_block128_grouped_swiglu (%d, %d) %s: largest err / bound %.3f, scales %.3f" % (I, K, form, ratio, scale_ratio))
    assert bool(torch.isfinite(h[:sum(SIZES)]).all()) and ratio <= 1.0 and scale_ratio <= 1.0, (ratio, scale_ratio)


@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", KS)
def test_integer_inputs_give_the_quantisers_bits_and_other_rows_keep_theirs(built, dev, K, form, pow2):
    a, sa, b, sb, want = exact(K)
    h, hs = fused(a, sa, b, sb, offsets(SIZES), form, pow2)
    for e, r0, r1 in groups(SIZES):
        codes, scales = gr.quant_a(want[e], pow2)
        assert torch.equal(hs[GUARD + r0:GUARD + r1], bits(scales)), e
        assert torch.equal(h[GUARD + r0:GUARD + r1], bits(codes)), e
    for t, fill in ((h, CODE_FILL), (hs, SCALE_FILL)):  # guards and the trailing rows
        assert bool((t[:GUARD] == fill).all()) and bool((t[GUARD + sum(SIZES):] == fill).all())


@pytest.mark.parametrize("form", [None, "tile"])
def test_one_captured_graph_replays_over_two_offset_arrays(built, dev, form):
    c, (a, sa, b, sb, _) = pkg(), gaussian(384)
    offs = (offsets(SIZES), offsets((65, 0, 1, 130, 17, 64, 0)))  # the same M_total, other owners for most rows
    ad, sad, bd, sbd, off = a.cuda(), sa.cuda(), b.cuda(), sb.cuda(), offs[0].cuda()
    h = torch.empty(a.shape[0], I, dtype=torch.uint8, device="cuda")
    hs = torch.empty(a.shape[0], I // 128, dtype=torch.int32, device="cuda")

    def step():
        c.gemm_fp8_block128_grouped_swiglu_fp8(ad, sad, bd, sbd, off, h.view(gr.F8), hs.view(torch.float32), form=form)

    def refill():
        h.fill_(CODE_FILL)
        hs.fill_(SCALE_FILL)
    eager = []
    for o in offs:
        off.copy_(o)
        refill()
        step()
        eager.append((h.cpu(), hs.cpu()))
    assert not torch.equal(eager[0][0], eager[1][0])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()  # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for i in (0, 1, 0, 1):
        off.copy_(offs[i])
        refill()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(h.cpu(), eager[i][0]) and torch.equal(hs.cpu(), eager[i][1]), i
