"""GPU: the causal FlashAttention-2 forward (cuda_learn_notes_amd.fa2_fwd_causal -> cln_fa2_fwd_causal, csrc/flash_attn_m16x_ext.hip)
against an fp64 masked softmax computed here on the CPU."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_AMPLIFIED_KEYS = 6e-3


def fa_tol(ref):
    """The scale rule of the plain attention names: 2^-9 max|O_ref| + 4e-4, never more than the amplified-key bound 6e-3."""
    return min(2.0 ** -9 * float(ref.abs().max()) + 4e-4, TOL_AMPLIFIED_KEYS)


def causal_ref(q, k, v, heads=None, rows=None):
    """fp64 O = softmax(Q K^T / sqrt(D) masked to key <= query) V on the CPU; optionally a subset of (flattened) heads and query rows."""
    B, H, N, D = q.shape
    qf, kf, vf = (t.reshape(B * H, N, D).double().cpu() for t in (q, k, v))
    hs = range(B * H) if heads is None else heads
    rs = torch.arange(N) if rows is None else torch.as_tensor(rows)
    out = []
    for h in hs:
        s = qf[h, rs] @ kf[h].T / D ** 0.5
        s = s.masked_fill(torch.arange(N)[None, :] > rs[:, None], float("-inf"))
        out.append(torch.softmax(s, dim=-1) @ vf[h])
    return torch.stack(out)


def qkv(B, H, N, D, seed=0, k_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, N, D, generator=g).half().cuda() for _ in range(3))
    if k_scale != 1.0:
        k = (k.float() * k_scale).half()
    return q, k, v


def run(q, k, v, stages=2):
    import cuda_learn_notes_amd as pkg
    o = torch.full_like(q, float("nan"))
    pkg.fa2_fwd_causal(q, k, v, o, stages)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("N", [256, 512, 2048])
@pytest.mark.parametrize("BH", [(1, 8), (2, 3)])  # H a multiple of 8 (heads pinned to XCDs) and not
def test_causal_parity(built, D, N, BH):
    q, k, v = qkv(*BH, N, D, seed=N + D)
    o = run(q, k, v)
    ref = causal_ref(q, k, v)
    err = (o.reshape(ref.shape).double().cpu() - ref).abs().max().item()
    assert err <= fa_tol(ref), (err, fa_tol(ref))


def test_causal_parity_large_grid(built):
    B, H, N, D = 2, 32, 4096, 128
    q, k, v = qkv(B, H, N, D, seed=7)
    o = run(q, k, v)
    heads, rows = [0, 13, 37, 63], list(range(0, N, 7)) + [N - 1]
    ref = causal_ref(q, k, v, heads, rows)
    got = o.reshape(B * H, N, D)[heads][:, rows].double().cpu()
    err = (got - ref).abs().max().item()
    assert err <= fa_tol(ref), (err, fa_tol(ref))


@pytest.mark.parametrize("D", [64, 128])
def test_stages_bit_identical(built, D):
    q, k, v = qkv(2, 8, 1024, D, seed=3)
    assert torch.equal(run(q, k, v, 1), run(q, k, v, 2))


@pytest.mark.parametrize("D", [64, 128])
def test_amplified_keys(built, D):
    q, k, v = qkv(1, 8, 1024, D, seed=11, k_scale=4.0)
    o = run(q, k, v)
    ref = causal_ref(q, k, v)
    err = (o.reshape(ref.shape).double().cpu() - ref).abs().max().item()
    assert err <= TOL_AMPLIFIED_KEYS, err


@pytest.mark.parametrize("D", [64, 128])
def test_row_zero_is_v_row_zero(built, D):
    q, k, v = qkv(2, 8, 512, D, seed=5)
    o = run(q, k, v)
    diff = (o[:, :, 0].float() - v[:, :, 0].float()).abs()
    ulp = torch.finfo(torch.float16).eps * torch.exp2(torch.floor(torch.log2(v[:, :, 0].float().abs().clamp_min(2.0 ** -14))))
    assert bool((diff <= ulp).all()), diff.max().item()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("i0", [127, 255, 300, 511])  # tile / row-block edges and inside a diagonal tile
def test_future_keys_do_not_leak(built, D, i0):
    q, k, v = qkv(1, 8, 1024, D, seed=21)
    base = run(q, k, v)
    g = torch.Generator().manual_seed(99)
    for amp in (1.0, 100.0):
        k2, v2 = k.clone(), v.clone()
        k2[:, :, i0 + 1:] = (torch.randn(k2[:, :, i0 + 1:].shape, generator=g) * amp).half().cuda()
        v2[:, :, i0 + 1:] = (torch.randn(v2[:, :, i0 + 1:].shape, generator=g) * amp).half().cuda()
        o = run(q, k2, v2)
        assert torch.equal(o[:, :, :i0 + 1], base[:, :, :i0 + 1]), (amp, i0)
        assert bool(torch.isfinite(o).all())


@pytest.mark.parametrize("D", [64, 128])
def test_last_row_matches_the_plain_kernel(built, D):
    B, H, N = 1, 8, 1024
    q, k, v = qkv(B, H, N, D, seed=31)
    o = run(q, k, v)
    plain = torch.zeros_like(q)
    built.flash_attn_lib().flash_attn_mma_stages_split_q_shared_qkv(q, k, v, plain, 2)
    torch.cuda.synchronize()
    ref = causal_ref(q, k, v, rows=[N - 1])
    err = (o[:, :, N - 1].float() - plain[:, :, N - 1].float()).abs().max().item()
    assert err <= 2 * fa_tol(ref), err


def test_unsupported_shapes_raise(built):
    import cuda_learn_notes_amd as pkg
    for (N, D) in ((256, 96), (256, 32), (384, 64), (128, 128)):
        q = torch.zeros(1, 8, N, D, dtype=torch.half, device="cuda")
        with pytest.raises(RuntimeError):
            pkg.fa2_fwd_causal(q, q, q, torch.zeros_like(q))
    with pytest.raises(RuntimeError):
        pkg.fa2_fwd_causal(*(torch.zeros(1, 8, 256, 64, dtype=torch.float32, device="cuda") for _ in range(4)))


@pytest.mark.parametrize("D", [64, 128])
def test_repeatable_and_graph_capture(built, D):
    import cuda_learn_notes_amd as pkg
    q, k, v = qkv(2, 8, 2048, D, seed=41)
    first = run(q, k, v)
    outs = [torch.empty_like(q) for _ in range(20)]
    for o in outs:
        pkg.fa2_fwd_causal(q, k, v, o)
    torch.cuda.synchronize()
    assert all(torch.equal(o, first) for o in outs)
    og = torch.zeros_like(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pkg.fa2_fwd_causal(q, k, v, og)  # warm-up outside the capture (first-call LDS attribute)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    og.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pkg.fa2_fwd_causal(q, k, v, og)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(og, first)
