"""GPU: the grouped (MoE) block-scaled FP8 GEMM (csrc/gemm_fp8_block128_grouped.*; DESIGN 4.4.28 has the largest err / bound seen per case)
against tests/gemm_fp8_block128_reference.py, per expert: fp64 under the derived bound, exact integer answers with every row of no expert
untouched, the bits of the dense entry on each expert alone, weights past 2^32 bytes, and one captured graph over two offset arrays. One
case set: E = 7 with sizes (0, 1, 17, 65, 130, 0, 64) and 3 trailing rows of no expert -- empty first, middle and next-to-last experts, a
one-row expert, starts off every 16- and 128-row boundary, one expert over two tiles from an unaligned start, an exact 64-row expert."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fp8_block128_reference as gr  # noqa: E402
from test_gpu_gemm_fp8_block128 import FILL, bits, gemm, pkg  # noqa: E402
pytestmark = pytest.mark.gpu

BF, F8 = gr.BF, gr.F8
SIZES, TRAIL, GUARD = (0, 1, 17, 65, 130, 0, 64), 3, 2
NK = ((264, 384), (136, 1024))  # a partial last N scale block with K/128 = 3 below the four-block ring; the ring wrapping twice
FORMS = ("skinny", "tile", None)


def offsets(sizes):
    return torch.tensor([0] + list(sizes), dtype=torch.int32).cumsum(0).to(torch.int32)


def groups(sizes):
    """(e, first row, end row) of the non-empty experts."""
    off = offsets(sizes).tolist()
    return [(e, off[e], off[e + 1]) for e in range(len(sizes)) if off[e + 1] > off[e]]


@functools.lru_cache(maxsize=None)
def gaussian(N, K):
    """a, sa of sum(SIZES) + TRAIL Gaussian rows, per expert its own quantised 0.05 randn weight, and per non-empty expert (ref, S) in fp64."""
    g = torch.Generator().manual_seed(1009 * N + K)
    a, sa = gr.quant_a(torch.randn(sum(SIZES) + TRAIL, K, generator=g).to(BF))
    b, sb = zip(*(gr.quant_b(0.05 * torch.randn(N, K, generator=g)) for _ in SIZES))
    refs = {e: gr.ref(a[r0:r1], sa[r0:r1], b[e], sb[e]) for e, r0, r1 in groups(SIZES)}
    return a, sa, torch.stack(b), torch.stack(sb), refs


@functools.lru_cache(maxsize=None)
def exact(N, K):
    """gr.exact per expert (its seed moves with M_e: other weights for every expert; an empty expert and the trailing rows get a case of
    their own that no answer may show), and per non-empty expert the bf16 answer."""
    cases = [gr.exact(m if m else 5 + e, N, K) for e, m in enumerate(SIZES)] + [gr.exact(TRAIL, N, K)]
    rows = [c for c, m in zip(cases, SIZES + (TRAIL,)) if m]
    want = {e: cases[e][4] for e, _, _ in groups(SIZES)}
    return (torch.cat([c[0] for c in rows]), torch.cat([c[1] for c in rows]), torch.stack([c[2] for c in cases[:-1]]),
            torch.stack([c[3] for c in cases[:-1]]), want)


def grouped(a, sa, b, sb, off, form):
    """The whole sentinel-filled tensor [GUARD + M_total + GUARD, N] whose middle rows were `out`, copied back."""
    M, N = a.shape[0], b.shape[1]
    whole = torch.full((GUARD + M + GUARD, N), FILL, dtype=torch.int16, device="cuda").view(BF)
    pkg().gemm_fp8_block128_grouped_bf16(a.cuda(), sa.cuda(), b.cuda(), sb.cuda(), off.cuda(), whole[GUARD:GUARD + M], form=form)
    torch.cuda.synchronize()
    return whole.cpu()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N,K", NK)
def test_each_expert_against_fp64_under_the_derived_bound(built, dev, N, K, form):
    a, sa, b, sb, refs = gaussian(N, K)
    out = grouped(a, sa, b, sb, offsets(SIZES), form)[GUARD:-GUARD].double()
    ratio = max(float(((out[r0:r1] - refs[e][0]).abs() / gr.bound(*refs[e], K)).max()) for e, r0, r1 in groups(SIZES))
    print("gemm_fp8_block128_grouped (%d, %d) %s: largest err / bound %.3f" % (N, K, form, ratio))
    assert bool(torch.isfinite(out[:sum(SIZES)]).all()) and ratio <= 1.0, ratio


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N,K", NK)
def test_integer_codes_are_exact_and_rows_of_no_expert_keep_their_bits(built, dev, N, K, form):
    a, sa, b, sb, want = exact(N, K)
    whole = bits(grouped(a, sa, b, sb, offsets(SIZES), form))
    for e, r0, r1 in groups(SIZES):
        assert torch.equal(whole[GUARD + r0:GUARD + r1], bits(want[e])), e
    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + sum(SIZES):] == FILL).all())  # guards and the trailing rows


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N,K", NK)
def test_each_experts_rows_carry_the_bits_of_the_dense_entry_on_it_alone(built, dev, N, K, form):
    a, sa, b, sb, _ = gaussian(N, K)
    out = bits(grouped(a, sa, b, sb, offsets(SIZES), form))[GUARD:-GUARD]
    for e, r0, r1 in groups(SIZES):
        assert torch.equal(out[r0:r1], bits(gemm(a[r0:r1], sa[r0:r1], b[e], sb[e]))), e


@pytest.mark.parametrize("form", [None, "tile"])
def test_expert_weights_past_2_to_the_32_bytes(built, dev, form):
    E, N, K = 33, 16384, 8192  # expert 32 starts 4.29e9 bytes into b
    torch.cuda.empty_cache()   # what earlier tests left in torch's cache counts as free
    if torch.cuda.mem_get_info()[0] < E * N * K + (1 << 30):
        pytest.skip("needs %.1f GB of free device memory" % ((E * N * K + (1 << 30)) * 1e-9))
    g = torch.Generator().manual_seed(33)
    b = torch.empty(E, N, K, dtype=torch.uint8, device="cuda").view(F8)  # uninitialised but for experts 0 and 32
    sb = torch.ones(E, N // 128, K // 128)
    a = torch.randint(-4, 5, (2, K), generator=g).float()
    sa = 2.0 ** torch.randint(-2, 3, (2, K // 128), generator=g).float()
    want = []
    for row, e in enumerate((0, E - 1)):
        w = torch.randint(-4, 5, (N, K), generator=g, dtype=torch.int8).float()
        b[e] = w.to(F8).cuda()
        want.append((a[row] * sa[row].repeat_interleave(128)) @ w.T)  # multiples of 1/4 below 2^20: exact in fp32 in any order
    off = torch.tensor([0] + [1] * (E - 1) + [2], dtype=torch.int32)
    out = torch.full((2, N), FILL, dtype=torch.int16, device="cuda").view(BF)
    pkg().gemm_fp8_block128_grouped_bf16(a.to(F8).cuda(), sa.cuda(), b, sb.cuda(), off.cuda(), out, form=form)
    assert torch.equal(bits(out.cpu()), bits(torch.stack(want).to(BF)))


@pytest.mark.parametrize("form", [None, "tile"])
def test_one_captured_graph_replays_over_two_offset_arrays(built, dev, form):
    c, (a, sa, b, sb, _) = pkg(), gaussian(264, 384)
    offs = (offsets(SIZES), offsets((65, 0, 1, 130, 17, 64, 0)))  # the same M_total, other owners for most rows
    ad, sad, bd, sbd, off = a.cuda(), sa.cuda(), b.cuda(), sb.cuda(), offs[0].cuda()
    out = torch.empty(a.shape[0], 264, dtype=BF, device="cuda")

    def step():
        c.gemm_fp8_block128_grouped_bf16(ad, sad, bd, sbd, off, out, form=form)
    eager = []
    for o in offs:
        off.copy_(o)
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
        off.copy_(offs[i])
        out.view(torch.int16).fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out.cpu()), bits(eager[i])), i
