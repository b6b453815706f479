"""GPU: the attention forward with log-sum-exp (fa2_fwd_lse -> cln_fa2_fwd_lse / cln_fa2_fwd_causal_lse, csrc/flash_attn_m16x_ext.hip), the
backward (fa2_bwd -> cln_fa2_bwd / cln_fa2_bwd_causal, csrc/flash_attn_bwd.hip) and the autograd function fa2_attention, against fp64 CPU
autograd of the (masked) softmax attention and torch SDPA's fp16 backward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


def qkv(B, H, N, D, seed=0, k_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, H, N, D, generator=g).half().cuda() for _ in range(4))
    if k_scale != 1.0:
        k = (k.float() * k_scale).half()
    return q, k, v, do


def fwd(q, k, v, causal, stages=2):
    import cuda_learn_notes_amd as pkg
    o = torch.full_like(q, float("nan"))
    lse = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device=q.device)
    pkg.fa2_fwd_lse(q, k, v, o, lse, causal=causal, stages=stages)
    torch.cuda.synchronize()
    return o, lse


def bwd(q, k, v, o, do, lse, causal):
    import cuda_learn_notes_amd as pkg
    dq, dk, dv = (torch.full_like(q, float("nan")) for _ in range(3))
    delta = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device=q.device)
    pkg.fa2_bwd(q, k, v, o, do, lse, dq, dk, dv, delta=delta, causal=causal)
    torch.cuda.synchronize()
    return dq, dk, dv, delta


def ref64(q, k, v, do, causal, heads=None):
    """fp64 CPU: lse, O and (dQ, dK, dV) of softmax(Q K^T / sqrt(D), masked to key <= query when causal) V, per flattened head."""
    B, H, N, D = q.shape
    hs = list(range(B * H)) if heads is None else list(heads)
    flat = [t.reshape(B * H, N, D)[hs].double().cpu() for t in (q, k, v, do)]
    qd, kd, vd = (t.requires_grad_() for t in flat[:3])
    s = qd @ kd.transpose(-1, -2) / D ** 0.5
    if causal:
        s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    o = torch.softmax(s, dim=-1) @ vd
    o.backward(flat[3])
    return lse.detach(), o.detach(), qd.grad, kd.grad, vd.grad


def sdpa_grads(q, k, v, do, causal, heads=None):
    B, H, N, D = q.shape
    qs, ks, vs = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, is_causal=causal)
    o.backward(do)
    hs = list(range(B * H)) if heads is None else list(heads)
    return [t.grad.reshape(B * H, N, D)[hs].double().cpu() for t in (qs, ks, vs)]


def check_grads(got, ref, sdpa, what):
    """The tolerance rule for each gradient X: max|X - X64| <= 2 max|X_sdpa - X64| + 2^-9 max|X64|. Calibrated on seeds these tests do not
    use (profiles/r08_fa_bwd_tol_calibration.log): the largest max|X - X64| / max|X64| seen was 1.65e-3 < 2^-9; 2^-10 was not enough
    without the causal mask, where the fp16 pre-scaled Q of the score recompute (shared with the forward) dominates."""
    for name, x, x64, xs in zip(("dQ", "dK", "dV"), got, ref, sdpa):
        assert bool(torch.isfinite(x).all()), (what, name)
        err = (x - x64).abs().max().item()
        bound = 2 * (xs - x64).abs().max().item() + 2.0 ** -9 * x64.abs().max().item()
        assert err <= bound, (what, name, err, bound)


def check_lse(lse, q, k, causal, l64, heads=None):
    """Against the fp64 logsumexp of the true scores (the fp16 rounding of the pre-scaled Q moves it by up to ~2^-10 relative), and tightly
    against the fp64 logsumexp of the scores the kernel forms: fp16(Q * fp16(log2 e / sqrt D)) . K, times ln 2."""
    B, H, N, D = q.shape
    got = flat(lse, heads)
    assert (got - l64).abs().max().item() <= 2.0 ** -10 * max(1.0, l64.abs().max().item())
    hs = list(range(B * H)) if heads is None else list(heads)
    sc = torch.tensor(LOG2E / D ** 0.5, dtype=torch.half)
    qs = (q.reshape(B * H, N, D)[hs].cpu() * sc).double()
    s = qs @ k.reshape(B * H, N, D)[hs].double().cpu().transpose(-1, -2) / LOG2E
    if causal:
        s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), float("-inf"))
    lk = torch.logsumexp(s, dim=-1)
    assert (got - lk).abs().max().item() <= 1e-5 * max(1.0, lk.abs().max().item())


def flat(t, heads=None):
    B, H, N = t.shape[:3]
    f = t.reshape(B * H, N, *t.shape[3:])
    return (f if heads is None else f[list(heads)]).double().cpu()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("N", [256, 512, 2048])
@pytest.mark.parametrize("BH", [(1, 8), (2, 3)])
def test_lse_delta_and_gradients(built, causal, D, N, BH):
    q, k, v, do = qkv(*BH, N, D, seed=1000 + N + D + int(causal))
    o, lse = fwd(q, k, v, causal)
    dq, dk, dv, delta = bwd(q, k, v, o, do, lse, causal)
    l64, o64, dq64, dk64, dv64 = ref64(q, k, v, do, causal)
    check_lse(lse, q, k, causal, l64)
    d32 = (do.float() * o.float()).sum(-1)
    assert torch.allclose(delta, d32, rtol=1e-5, atol=1e-5 * float(d32.abs().max())), (delta - d32).abs().max().item()
    check_grads([flat(x) for x in (dq, dk, dv)], (dq64, dk64, dv64), sdpa_grads(q, k, v, do, causal), (causal, D, N, BH))


@pytest.mark.parametrize("causal", [False, True])
def test_large_grid_sampled_heads(built, causal):
    B, H, N, D = 2, 32, 4096, 128
    q, k, v, do = qkv(B, H, N, D, seed=77)
    o, lse = fwd(q, k, v, causal)
    dq, dk, dv, _ = bwd(q, k, v, o, do, lse, causal)
    heads = [0, 13, 37, 63]
    l64, _, dq64, dk64, dv64 = ref64(q, k, v, do, causal, heads)
    check_lse(lse, q, k, causal, l64, heads)
    check_grads([flat(x, heads) for x in (dq, dk, dv)], (dq64, dk64, dv64), sdpa_grads(q, k, v, do, causal, heads), "large")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_amplified_keys(built, causal, D):
    q, k, v, do = qkv(1, 8, 1024, D, seed=2024 + D, k_scale=4.0)
    o, lse = fwd(q, k, v, causal)
    dq, dk, dv, _ = bwd(q, k, v, o, do, lse, causal)
    l64, _, dq64, dk64, dv64 = ref64(q, k, v, do, causal)
    check_lse(lse, q, k, causal, l64)
    check_grads([flat(x) for x in (dq, dk, dv)], (dq64, dk64, dv64), sdpa_grads(q, k, v, do, causal), "amplified")


@pytest.mark.parametrize("D", [64, 128])
def test_causal_lse_output_is_the_causal_forward(built, D):
    import cuda_learn_notes_amd as pkg
    q, k, v, _ = qkv(2, 8, 1024, D, seed=5)
    o, _ = fwd(q, k, v, True)
    plain = torch.zeros_like(q)
    pkg.fa2_fwd_causal(q, k, v, plain)
    torch.cuda.synchronize()
    assert torch.equal(o, plain)


@pytest.mark.parametrize("D", [64, 128])
def test_plain_lse_output_is_the_plain_forward(built, D):
    import cuda_learn_notes_amd as pkg
    name = "flash_attn_mma_stages_split_q_shared_qkv"
    q, k, v, _ = qkv(2, 8, 1024, D, seed=6)
    o, _ = fwd(q, k, v, False)
    plain = torch.zeros_like(q)
    getattr(built.flash_attn_lib(), name)(q, k, v, plain, 2)
    torch.cuda.synchronize()
    text = pkg.manifest.describe(name, tuple(q.shape), 2)
    if text.startswith("fa2_fwd_m16x<") and "pre-scaled Q" in text and "x 32 rows" in text:
        assert torch.equal(o, plain), text
    else:
        ref = ref64(q, k, v, torch.zeros_like(q), False)[1]
        tol = min(2.0 ** -9 * float(ref.abs().max()) + 4e-4, 6e-3)  # fa_tol of the plain names
        assert (flat(o) - ref).abs().max().item() <= tol
        assert (flat(plain) - ref).abs().max().item() <= tol


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_stages_bit_identical(built, causal, D):
    q, k, v, _ = qkv(1, 8, 1024, D, seed=8)
    o1, l1 = fwd(q, k, v, causal, stages=1)
    o2, l2 = fwd(q, k, v, causal, stages=2)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_backward_is_deterministic(built, causal, D):
    q, k, v, do = qkv(2, 8, 2048, D, seed=9)
    o, lse = fwd(q, k, v, causal)
    runs = [bwd(q, k, v, o, do, lse, causal) for _ in range(3)]
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))


@pytest.mark.parametrize("causal", [False, True])
def test_autograd_matches_direct_backward(built, causal):
    import cuda_learn_notes_amd as pkg
    q, k, v, do = qkv(2, 4, 512, 64, seed=10)
    o, lse = fwd(q, k, v, causal)
    dq, dk, dv, _ = bwd(q, k, v, o, do, lse, causal)
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    out = pkg.fa2_attention(qa, ka, va, causal=causal)
    assert torch.equal(out, o)
    g = torch.empty(2, 4, 64, 512, dtype=torch.half, device="cuda").transpose(-1, -2)  # non-contiguous grad_out
    g.copy_(do)
    out.backward(g)
    torch.cuda.synchronize()
    assert torch.equal(qa.grad, dq) and torch.equal(ka.grad, dk) and torch.equal(va.grad, dv)


def test_autograd_on_a_side_stream(built):
    import cuda_learn_notes_amd as pkg
    q, k, v, do = qkv(1, 8, 1024, 128, seed=12)
    o, lse = fwd(q, k, v, True)
    dq, dk, dv, _ = bwd(q, k, v, o, do, lse, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
        out = pkg.fa2_attention(qa, ka, va, causal=True)
        out.backward(do)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(out, o)
    assert torch.equal(qa.grad, dq) and torch.equal(ka.grad, dk) and torch.equal(va.grad, dv)


def test_python_errors(built):
    import cuda_learn_notes_amd as pkg
    x = torch.zeros(1, 8, 256, 64, dtype=torch.half)
    lse = torch.zeros(1, 8, 256)
    with pytest.raises(RuntimeError):
        pkg.fa2_fwd_lse(x, x, x, x.clone(), lse)  # CPU tensors
    with pytest.raises(RuntimeError):
        pkg.fa2_bwd(x, x, x, x, x, lse, x.clone(), x.clone(), x.clone())
    for (N, D, dt) in ((256, 96, torch.half), (384, 64, torch.half), (256, 64, torch.float32)):
        q = torch.zeros(1, 8, N, D, dtype=dt, device="cuda")
        lg = torch.zeros(1, 8, N, device="cuda")
        outs = [torch.zeros_like(q) for _ in range(4)]
        with pytest.raises(RuntimeError):
            pkg.fa2_fwd_lse(q, q, q, outs[0], lg)
        with pytest.raises(RuntimeError):
            pkg.fa2_bwd(q, q, q, q, q, lg, *outs[1:], causal=True)
        with pytest.raises(RuntimeError):
            pkg.fa2_attention(q, q, q)
