"""CPU only: the fp64 references of tests/fa_reference.py, proven before they judge a kernel (tests/test_gpu_fa2_edges.py) -- the chunked
closed-form backward against fp64 autograd, the chunked kernel-score log-sum-exp against the unchunked expression of check_lse, the
one-hot problem against its exact answers, and the closed forms the GPU tests rely on."""
import math

import pytest
import torch

import fa_reference as far

NAMES = ("lse", "O", "dQ", "dK", "dV")
ONEHOT_SHAPES = [(768, 64), (4096, 64), (768, 128), (4096, 128)]  # every (N, D) of test_gpu_fa2_edges.py::test_onehot_attention


def gauss(B, H, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, N, D, generator=g).half() for _ in range(4)]


def autograd64(q, k, v, do, causal, heads=None):
    """The formula of ref64 in tests/test_gpu_fa2_bwd.py."""
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


def rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize("chunk", [256, 1024])  # divides N = 256 and 768 / does not divide 768, exceeds 256
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,D", [(256, 64), (768, 64), (256, 128), (768, 128)])
def test_ref_chunked_is_the_autograd_reference(N, D, causal, chunk):
    q, k, v, do = gauss(1, 3, N, D, seed=N + D + int(causal))
    want = autograd64(q, k, v, do, causal)
    for c in (chunk, 200):  # 200 divides neither N
        got = far.ref_chunked(q, k, v, do, causal, chunk=c)
        for name, a, b in zip(NAMES, got, want):
            assert a.shape == b.shape and a.dtype == torch.float64
            assert rel(a, b) <= 1e-12, (name, c, rel(a, b))


def test_ref_chunked_head_subset():
    q, k, v, do = gauss(2, 3, 256, 64, seed=3)
    full = far.ref_chunked(q, k, v, do, True)
    part = far.ref_chunked(q, k, v, do, True, heads=[4, 1])
    for a, b in zip(part, full):
        assert torch.equal(a, b[[4, 1]])


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,D", [(256, 64), (768, 128)])
def test_kernel_scores_lse_is_the_expression_of_check_lse(N, D, causal):
    q, k, _, _ = gauss(2, 2, N, D, seed=11 + N)
    heads = [0, 3]
    sc = torch.tensor(far.LOG2E / D ** 0.5, dtype=torch.half)
    qs = (q.reshape(4, N, D)[heads].cpu() * sc).double()
    s = qs @ k.reshape(4, N, D)[heads].double().cpu().transpose(-1, -2) / far.LOG2E
    if causal:
        s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), float("-inf"))
    lk = torch.logsumexp(s, dim=-1)
    assert torch.equal(far.kernel_scores_lse(q, k, causal, heads, chunk=N), lk)
    assert rel(far.kernel_scores_lse(q, k, causal, heads, chunk=200), lk) <= 1e-13
    # and it is a different number from the logsumexp of the true scores: the fp16 rounding of the pre-scaled Q is in it
    l64 = far.ref_chunked(q, k, k, k, causal, heads)[0]
    assert 1e-6 < (lk - l64).abs().max().item() <= 2.0 ** -10 * max(1.0, l64.abs().max().item())
    # check_lse itself accepts both references and refuses a shifted LSE
    far.check_lse(lk.float().reshape(1, 2, N), q.reshape(4, N, D)[heads].reshape(1, 2, N, D), k.reshape(4, N, D)[heads].reshape(1, 2, N, D), causal, l64)
    with pytest.raises(AssertionError):
        far.check_lse((lk + 1e-4 * max(1.0, lk.abs().max().item())).float().reshape(1, 2, N), q.reshape(4, N, D)[heads].reshape(1, 2, N, D),
                      k.reshape(4, N, D)[heads].reshape(1, 2, N, D), causal, l64)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,D", ONEHOT_SHAPES)
def test_onehot_problem_has_its_exact_answers(N, D, causal):
    q, k, v, do, pi = far.onehot_problem(N, D, causal, seed=N + D)
    for t in (q, k, v, do):
        assert t.dtype == torch.half and t.shape == (N, D)
    bits = (N - 1).bit_length()
    r = D // bits
    assert set(k.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(q.unique().tolist()) <= {-16.0, 0.0, 16.0}
    assert int((k != 0).sum()) == N * r * bits and len({tuple(row) for row in k[:, :bits].tolist()}) == N  # full codes, all distinct
    assert torch.equal(q, k[pi] * 16)
    assert not torch.equal(v, do)
    for t in (v, do):  # N(0, 1)
        assert abs(t.float().std().item() - 1.0) < 0.05 and abs(t.float().mean().item()) < 0.05
    if causal:
        assert bool((pi <= torch.arange(N)).all()) and bool((pi >= 0).all())
        assert pi.unique().numel() > N // 4  # not the constant map
    else:
        assert torch.equal(pi.sort().values, torch.arange(N))
        assert not torch.equal(pi, torch.arange(N))
    assert not torch.equal(pi, far.onehot_problem(N, D, causal, seed=N + D + 1)[4])  # seeded
    lse, o, dq, dk, dv = (t[0] for t in far.ref_chunked(*(t[None, None] for t in (q, k, v, do)), causal))
    s_t = (q.double() * k[pi].double()).sum(-1) / D ** 0.5
    assert s_t.min().item() == pytest.approx(16 * r * bits / D ** 0.5, rel=1e-14)
    mass = -torch.expm1(s_t - lse)  # 1 - P[i, pi(i)]
    assert 0.0 <= mass.min().item() and mass.max().item() <= 1e-7, mass.max().item()
    assert (o - v[pi].double()).abs().max().item() <= 1e-6
    assert (dv - torch.zeros(N, D, dtype=torch.float64).index_add_(0, pi, do.double())).abs().max().item() <= 1e-6
    assert (lse - s_t).abs().max().item() <= 1e-6
    # dQ and dK are ~0 next to dV: the bound of the GPU test, 2^-9 max|dV64|, is far above the true values
    assert max(dq.abs().max().item(), dk.abs().max().item()) <= 1e-3 * 2.0 ** -9 * dv.abs().max().item()


def test_onehot_problem_refuses_a_gap_under_20_nats():
    with pytest.raises(AssertionError):
        far.onehot_problem(16384, 64, False, seed=0)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_closed_forms_with_zero_queries(D, causal):
    N = 1024
    _, k, v, do = gauss(1, 2, N, D, seed=5 + D)
    lse, o, dq, dk, dv = far.ref_chunked(torch.zeros_like(k), k, v, do, causal, chunk=256)
    vd = v.reshape(2, N, D).double()
    if causal:
        cnt = torch.arange(1, N + 1, dtype=torch.float64)
        assert (lse - cnt.log()).abs().max().item() <= 1e-12
        assert (o - vd.cumsum(1) / cnt[None, :, None]).abs().max().item() <= 1e-12
    else:
        assert (lse - math.log(N)).abs().max().item() <= 1e-12
        assert (o - vd.mean(1, keepdim=True)).abs().max().item() <= 1e-12
    assert torch.equal(dk, torch.zeros_like(dk))
    assert dq.abs().max().item() > 1e-3 and dv.abs().max().item() > 1e-3  # those two are not trivial


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_gradient_sum_identities(D, causal):
    N = 1024
    q, k, v, do = gauss(1, 2, N, D, seed=9 + D)
    _, _, _, dk, dv = far.ref_chunked(q, k, v, do, causal, chunk=256)
    # softmax shift invariance: adding one vector to every key changes no output, so sum_j dK_j = 0
    assert (dk.sum(1).abs() / dk.abs().sum(1)).max().item() <= 1e-12
    if not causal:  # every row of P sums to 1 over all keys
        want = do.reshape(2, N, D).double().sum(1)
        assert ((dv.sum(1) - want).abs() / dv.abs().sum(1)).max().item() <= 1e-12
    # what test_gpu_fa2_edges.py::test_key_gradients_sum_to_zero relies on: fp16 rounding of dK alone stays within 2^-11 sum_j |dK_j|
    assert bool((dk.half().double().sum(1).abs() <= 2.0 ** -11 * dk.abs().sum(1)).all())


def test_constant_values_give_that_row():
    N, D = 512, 64
    q, k, _, do = gauss(1, 2, N, D, seed=21)
    v = torch.randn(1, 2, 1, D, generator=torch.Generator().manual_seed(22)).half().expand(1, 2, N, D)
    for causal in (False, True):
        o = far.ref_chunked(q, k, v, do, causal)[1]
        assert (o - v.reshape(2, N, D).double()).abs().max().item() <= 1e-14


def test_tolerance_rules_are_those_of_the_attention_tests():
    """fa_tol, check_grads, check_lse and flat are copies: the source text of each equals that of its original."""
    import ast
    import os
    here = os.path.dirname(os.path.abspath(__file__))

    def funcs(path):
        src = open(os.path.join(here, path)).read()
        return {n.name: ast.get_source_segment(src, n) for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}

    mine, bwd, causal = funcs("fa_reference.py"), funcs("test_gpu_fa2_bwd.py"), funcs("test_gpu_fa2_causal.py")
    assert mine["fa_tol"] == causal["fa_tol"]
    for name in ("check_grads", "check_lse", "flat"):
        assert mine[name] == bwd[name], name
