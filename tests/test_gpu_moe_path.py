"""GPU: the MoE token path (csrc/moe_*.{cuh,hip}; DESIGN 4.4.33 has the largest err / bound seen) against tests/moe_reference.py and the
quantisers' references: exact ids and derived weight bounds for the router, exact answers inside guard words for the sort, the quantisers'
bits for the dispatch, exact and fp64-bounded sums for the combine, and the whole path in one captured graph."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fp8_block128_reference as gr  # noqa: E402
import gemm_mxfp4_reference as mr  # noqa: E402
import moe_reference as mo  # noqa: E402
pytestmark = pytest.mark.gpu

BF, F8, E8, F32, I32 = mo.BF, mr.F8, mr.E8, mo.F32, mo.I32
G, FILL = 16, 0x5A  # guard elements on both sides of an output; the byte no kernel writes there


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def guarded(shape, dtype):
    """(whole, view): a byte-FILL-ed flat tensor with G guard elements on both sides of the contiguous `view` of `shape`."""
    n = int(torch.tensor(shape).prod())
    whole = torch.full(((n + 2 * G) * torch.empty(0, dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device="cuda").view(dtype)
    return whole, whole[G:G + n].view(shape)


def guards_hold(whole):
    b = whole.view(torch.uint8).cpu()
    g = G * whole.element_size()
    return bool((b[:g] == FILL).all()) and bool((b[-g:] == FILL).all())


@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("T,E,k", [(1, 8, 2), (5, 128, 4), (67, 256, 8), (3, 512, 10), (4, 60, 4)])
def test_route_ids_are_the_stable_fp64_sort_and_weights_are_inside_the_bound(built, dev, T, E, k, dtype, scoring):
    logits, bias, keys, s = mo.route_case(T, E, k, scoring)
    for renorm, scale in ((True, 1.0), (False, 2.5)):
        want_ids, want_w, bound = mo.route_ref(logits, keys, s, k, renorm, scale)
        (wi, ids), (ww, w) = guarded((T, k), I32), guarded((T, k), F32)
        pkg().moe_route_topk(logits.to(dtype).cuda(), ids, w, scoring, None if bias is None else bias.cuda(), renorm, scale)
        assert torch.equal(ids.cpu(), want_ids) and guards_hold(wi) and guards_hold(ww)
        ratio = float(((w.cpu().double() - want_w).abs() / bound).max())
        print("moe_route_topk (%d, %d, %d) %s renorm=%d: largest err / bound %.3f" % (T, E, k, scoring, renorm, ratio))
        assert ratio <= 1.0, ratio


@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
def test_route_equal_keys_go_to_the_lower_index(built, dev, scoring):
    logits, bias, _, _ = mo.route_case(3, 200, 6, scoring, tie=True)
    ids, w = torch.empty(3, 6, dtype=I32, device="cuda"), torch.empty(3, 6, device="cuda")
    pkg().moe_route_topk(logits.to(BF).cuda(), ids, w, scoring, None if bias is None else bias.cuda())
    assert torch.equal(ids.cpu(), torch.arange(6, dtype=I32).expand(3, 6))
    assert scoring == "sigmoid" or torch.equal(w.cpu(), torch.full((3, 6), 1 / 6))  # exp(0) = 1 six times: 1 / 6 rounded once


# The sizes below are multiples of the plan's chunk. Parameters are made at collection, before the library is built, so the chunk cannot be
# read from moe_sort_plan here: it is written out, and test_sort_plan_is_what_the_sizes_below_assume fails when the plan says otherwise.
CHUNK = 2048


def test_sort_plan_is_what_the_sizes_below_assume(built):
    assert pkg().moe_sort_plan(CHUNK, 5) == (1, CHUNK, 0) and pkg().moe_sort_plan(CHUNK + 1, 5) == (2, CHUNK, 40)


@pytest.mark.parametrize("pattern", ["uniform", "one", "holes"])
@pytest.mark.parametrize("E", [1, 5, 256, 2050])  # 2050: a second tile of experts in every kernel
@pytest.mark.parametrize("n", [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17])
def test_sort_equals_the_stable_cpu_sort_inside_guard_words(built, dev, n, E, pattern):
    ids = mo.sort_ids(n, E, pattern)
    want = mo.sort_ref(ids, E)
    outs = [guarded(s, I32) for s in ((E + 1,), (n,), (n, 1))]
    ws_bytes = pkg().moe_sort_plan(n, E)[2]
    wws, ws = guarded((max(ws_bytes // 4, 1),), I32)
    pkg().moe_sort(ids.view(n, 1).cuda(), E, outs[0][1], outs[1][1], outs[2][1], ws)
    for (whole, got), w in zip(outs, want):
        assert torch.equal(got.cpu().flatten(), w) and guards_hold(whole)
    assert guards_hold(wws)


T_D, K_D = 9, 3
SRC = torch.tensor([4, 26, -1, 0, 13, 27, 5, 5, -1, 22, 1 << 30, 8] + [-1] * 15, dtype=I32)  # dropped rows, 27 and 2^30 out of range, 5 twice


@pytest.mark.parametrize("K,kind", [(128, "fp8"), (384, "fp8"), (384, "fp8_pow2"), (128, "fp8_pow2"), (32, "mx"), (416, "mx"),
                                     (1152, "fp8"), (2880, "mx")])  # the last two: a row wider than a workgroup (blockIdx.y the piece)
def test_dispatch_rows_carry_the_quantisers_bits_and_dropped_rows_are_not_written(built, dev, K, kind):
    x = mr.quant_rows(T_D, max(K, 96))[:, :K].contiguous() if kind == "mx" else (gr.gaussian(T_D, 8, K)[0] * 3.0).to(BF)
    live = (SRC >= 0) & (SRC < T_D * K_D)
    rows = x[(SRC[live] // K_D).long()]
    want_c, want_s = mr.quant_a(rows) if kind == "mx" else gr.quant_a(rows, kind == "fp8_pow2")
    blk, sdt = (32, E8) if kind == "mx" else (128, F32)
    (wc, codes), (wsc, scales) = guarded((SRC.numel(), K), F8), guarded((SRC.numel(), K // blk), sdt)
    if kind == "mx":
        pkg().moe_dispatch_mxfp8_bf16(x.cuda(), SRC.cuda(), K_D, codes, scales)
    else:
        pkg().moe_dispatch_fp8_block128_bf16(x.cuda(), SRC.cuda(), K_D, codes, scales, kind == "fp8_pow2")
    cb, sb = codes.view(torch.uint8).cpu(), scales.cpu().contiguous().view(torch.uint8).view(SRC.numel(), -1)
    assert torch.equal(cb[live], want_c.view(torch.uint8)) and torch.equal(sb[live], want_s.contiguous().view(torch.uint8).view(rows.shape[0], -1))
    assert bool((cb[~live] == FILL).all()) and bool((sb[~live] == FILL).all()) and guards_hold(wc) and guards_hold(wsc)


def combine_case(T, k, N, exact):
    g = torch.Generator().manual_seed(T + 3 * k + N)
    M = T * k + 2
    pos = torch.randperm(M, generator=g)[:T * k].view(T, k).to(I32)
    pos[0, 0] = -1
    if T > 1:
        pos[T - 1, k - 1], pos[1, 0] = M, -7
    if exact:  # integers times powers of two: every partial sum is exact in fp32 and the total below 2^8, so exact in bf16
        y = torch.randint(-3, 4, (M, N), generator=g).to(BF)
        w = 2.0 ** torch.randint(-1, 2, (T, k), generator=g).float()
        res = torch.randint(-8, 9, (T, N), generator=g).to(BF)
    else:
        y, w, res = torch.randn(M, N, generator=g).to(BF), torch.rand(T, k, generator=g), torch.randn(T, N, generator=g).to(BF)
    return y, pos, w, res


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "gaussian"])
@pytest.mark.parametrize("T,k,N", [(1, 1, 8), (5, 4, 136), (67, 8, 2880)])
def test_combine_is_exact_on_integers_and_inside_the_fp64_bound_on_gaussians(built, dev, T, k, N, exact, with_res):
    y, pos, w, res = combine_case(T, k, N, exact)
    res = res if with_res else None
    want, S = mo.combine_ref(y, pos, w, res)
    whole, out = guarded((T, N), BF)
    pkg().moe_combine_bf16(y.cuda(), pos.cuda(), w.cuda(), out, None if res is None else res.cuda())
    got = out.cpu()
    assert guards_hold(whole)
    if exact:
        assert torch.equal(got.view(torch.int16), want.to(BF).view(torch.int16))
    else:
        bound = 2.0 ** -8 * want.abs() + k * 2.0 ** -23 * S
        assert float(((got.double() - want).abs() / bound.clamp_min(1e-30)).max()) <= 1.0


def test_one_captured_graph_from_logits_to_out_replays_the_eager_and_the_torch_fed_bits(built, dev):
    c = pkg()
    T, E, k, K, N = 33, 8, 2, 256, 136
    n = T * k
    x = gr.gaussian(T, N, K)[0].cuda()
    wq = [gr.quant_b(0.05 * torch.randn(N, K, generator=torch.Generator().manual_seed(e))) for e in range(E)]
    b, sb = (torch.stack([q[i] for q in wq]).cuda() for i in (0, 1))
    cases = [mo.route_case(T, E, k, "softmax")[0], mo.route_case(T, E, k + 1, "softmax")[0]]
    logits = torch.empty(T, E, dtype=BF, device="cuda")
    ids, w, pos = (torch.empty(T, k, dtype=d, device="cuda") for d in (I32, F32, I32))
    off, src = torch.empty(E + 1, dtype=I32, device="cuda"), torch.empty(n, dtype=I32, device="cuda")
    codes, scales = torch.empty(n, K, dtype=F8, device="cuda"), torch.empty(n, K // 128, device="cuda")
    y, out = torch.empty(n, N, dtype=BF, device="cuda"), torch.empty(T, N, dtype=BF, device="cuda")

    def step():
        c.moe_route_topk(logits, ids, w)
        c.moe_sort(ids, E, off, src, pos)
        c.moe_dispatch_fp8_block128_bf16(x, src, k, codes, scales)
        c.gemm_fp8_block128_grouped_bf16(codes, scales, b, sb, off, y)
        c.moe_combine_bf16(y, pos, w, out)
    eager = []
    for lg in cases:
        logits.copy_(lg)
        step()
        eager.append(out.cpu())
        # the same GEMM fed by torch's permutation and the existing quantiser
        order = torch.sort(ids.flatten().long(), stable=True).indices
        assert torch.equal(src.cpu().long(), order.cpu())
        c2, s2, y2 = torch.empty_like(codes), torch.empty_like(scales), torch.empty_like(y)
        c.quant_fp8_block128_bf16(x[order // k].contiguous(), c2, s2)
        c.gemm_fp8_block128_grouped_bf16(c2, s2, b, sb, off, y2)
        out2 = torch.empty_like(out)
        c.moe_combine_bf16(y2, pos, w, out2)
        assert torch.equal(y2.view(torch.int16), y.view(torch.int16)) and torch.equal(out2.cpu().view(torch.int16), eager[-1].view(torch.int16))
    assert not torch.equal(eager[0], eager[1])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()  # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for i in (0, 1, 0, 1):
        logits.copy_(cases[i])
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(torch.int16), eager[i].view(torch.int16)), i
