"""GPU: the attention forwards (fa2_fwd_causal, fa2_fwd_lse causal and not) and the backward (fa2_bwd) where the parity tests of
tests/test_gpu_fa2_causal.py / tests/test_gpu_fa2_bwd.py do not look: block counts that are not powers of two, N = 8192 / 16384, guard
bands around every tensor, causality and head independence of the backward bit for bit, a one-hot problem with exact answers and
scores of 120-170 nats, closed forms (Q = 0, constant V, sum_j dK_j = 0) and loss-scaled dO. References: tests/fa_reference.py (fp64,
proven by tests/test_fa_reference.py); tolerances: the rules of the two files above, unchanged. Every case prints `error / bound` per
output before it asserts (pytest -s); the figures of one MI355X run are profiles/r09_fa2_edge_tests.log."""
import math

import pytest
import torch

import fa_reference as far
from fa_reference import SENTINEL, guarded, pads  # noqa: F401

pytestmark = pytest.mark.gpu


def gauss(B, H, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, N, D, generator=g).half().cuda() for _ in range(4)]


def nan_like(t):
    return torch.full_like(t, float("nan"))


def fwd_causal(q, k, v, stages=2, o=None):
    import cuda_learn_notes_amd as pkg
    o = nan_like(q) if o is None else o
    pkg.fa2_fwd_causal(q, k, v, o, stages)
    torch.cuda.synchronize()
    return o


def fwd_lse(q, k, v, causal, stages=2, o=None, lse=None):
    import cuda_learn_notes_amd as pkg
    o = nan_like(q) if o is None else o
    lse = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device=q.device) if lse is None else lse
    pkg.fa2_fwd_lse(q, k, v, o, lse, causal=causal, stages=stages)
    torch.cuda.synchronize()
    return o, lse


def bwd(q, k, v, o, do, lse, causal, outs=None):
    import cuda_learn_notes_amd as pkg
    if outs is None:
        outs = [nan_like(q) for _ in range(3)] + [torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device=q.device)]
    dq, dk, dv, delta = outs
    pkg.fa2_bwd(q, k, v, o, do, lse, dq, dk, dv, delta=delta, causal=causal)
    torch.cuda.synchronize()
    return dq, dk, dv, delta


def run_all(q, k, v, do, causal):
    """(O, LSE, dQ, dK, dV, delta) of fa2_fwd_lse + fa2_bwd, all starting as NaN."""
    o, lse = fwd_lse(q, k, v, causal)
    return (o, lse) + tuple(bwd(q, k, v, o, do, lse, causal))


OUT_NAMES = ("O", "LSE", "dQ", "dK", "dV", "delta")


def sdpa_grads(q, k, v, do, causal, heads=None):
    B, H, N, D = q.shape
    qs, ks, vs = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, is_causal=causal)
    o.backward(do)
    hs = list(range(B * H)) if heads is None else list(heads)
    return [t.grad.reshape(B * H, N, D)[hs].double().cpu() for t in (qs, ks, vs)]


def report(what, name, err, bound):
    print("%-58s %-6s %.3e / %.3e = %.3f%s" % (what, name, err, bound, err / bound if bound > 0 else float("inf" if err > 0 else 0),
                                                "  OVER_HALF" if err > 0.5 * bound else ""))


def maxerr(a, b):
    return (a - b).abs().max().item()


def check_delta(delta, do, o, what):
    d32 = (do.float() * o.float()).sum(-1)
    diff, bound = (delta - d32).abs(), 1e-5 * float(d32.abs().max()) + 1e-5 * d32.abs()  # the rule is elementwise: report the worst element
    worst = (diff / bound).argmax()
    report(what, "delta", diff.flatten()[worst].item(), bound.flatten()[worst].item())
    assert torch.allclose(delta, d32, rtol=1e-5, atol=1e-5 * float(d32.abs().max())), (what, maxerr(delta, d32))


def check_case(what, q, k, v, do, causal, heads=None, outs=None):
    """Run the forwards and the backward on (q, k, v, do) and hold every output of `heads` (all when None) to the rules: fa_tol for O,
    check_lse's two bounds for LSE (the second through kernel_scores_lse, so N x N never exists), check_grads for dQ / dK / dV, delta
    against rowsum(dO o O) in fp32. `outs`: a finished run_all() of the same inputs. Returns that run."""
    N = q.shape[2]
    o, lse, dq, dk, dv, delta = run_all(q, k, v, do, causal) if outs is None else outs
    l64, o64, dq64, dk64, dv64 = far.ref_chunked(q, k, v, do, causal, heads)
    lk = far.kernel_scores_lse(q, k, causal, heads)
    sd = sdpa_grads(q, k, v, do, causal, heads)
    tol = far.fa_tol(o64)
    report(what, "O", maxerr(far.flat(o, heads), o64), tol)
    got = far.flat(lse, heads)
    b1, b2 = 2.0 ** -10 * max(1.0, l64.abs().max().item()), 1e-5 * max(1.0, lk.abs().max().item())
    report(what, "LSE", maxerr(got, l64), b1)
    report(what, "LSE_k", maxerr(got, lk), b2)
    grads = [far.flat(x, heads) for x in (dq, dk, dv)]
    for name, x, x64, xs in zip(("dQ", "dK", "dV"), grads, (dq64, dk64, dv64), sd):
        report(what, name, maxerr(x, x64), 2 * maxerr(xs, x64) + 2.0 ** -9 * x64.abs().max().item())
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
    assert maxerr(far.flat(o, heads), o64) <= tol, what
    if causal:
        oc = fwd_causal(q, k, v)
        report(what, "O_caus", maxerr(far.flat(oc, heads), o64), tol)
        assert maxerr(far.flat(oc, heads), o64) <= tol, what
    if N <= 4096:  # check_lse forms N x N scores per head: one head at a time (each head's bound is at most the joint one asserted below)
        for i, h in enumerate(range(q.shape[0] * q.shape[1]) if heads is None else heads):
            far.check_lse(lse, q, k, causal, l64[i:i + 1], [h])
    assert maxerr(got, l64) <= b1 and maxerr(got, lk) <= b2, what
    check_delta(delta, do, o, what)
    far.check_grads(grads, (dq64, dk64, dv64), sd, what)
    return o, lse, dq, dk, dv, delta


# ---- a. block counts that are not powers of two: 3, 5, 7, 13 forward blocks (256 rows), 6, 10, 14, 26 backward blocks (128 rows)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("N", [768, 1280, 1792, 3328])
@pytest.mark.parametrize("BH", [(1, 5), (3, 8)])
def test_odd_block_counts(built, causal, D, N, BH):
    what = "odd_blocks N=%d D=%d causal=%d BH=%s" % (N, D, causal, BH)
    q, k, v, do = gauss(*BH, N, D, seed=3000 + N + D + int(causal) + BH[1])
    o, lse = check_case(what, q, k, v, do, causal)[:2]
    o1, l1 = fwd_lse(q, k, v, causal, stages=1)
    assert torch.equal(o1, o) and torch.equal(l1, lse), what
    if causal:
        oc = fwd_causal(q, k, v)
        assert torch.equal(oc, o), what
        assert torch.equal(fwd_causal(q, k, v, stages=1), oc), what


# ---- b. long sequences


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("N", [8192, 16384])
def test_long_sequences(built, causal, D, N):
    q, k, v, do = gauss(1, 8, N, D, seed=5000 + N + D + int(causal))
    check_case("long N=%d D=%d causal=%d heads 0,7" % (N, D, causal), q, k, v, do, causal, heads=[0, 7])


# ---- c. guard bands: every tensor is batches 1..B of a [B + 2, ...] buffer; input pads NaN, output pads a finite sentinel

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("N", [256, 768])
def test_guard_bands(built, causal, D, N):
    B, H = 2, 3
    what = "guard N=%d D=%d causal=%d" % (N, D, causal)
    q, k, v, do = gauss(B, H, N, D, seed=7000 + N + D + int(causal))
    plain = run_all(q, k, v, do, causal) + ((fwd_causal(q, k, v),) if causal else ())
    ins = [guarded(t.shape, t.dtype, t)[1] for t in (q, k, v, do)]
    for g, t in zip(ins, (q, k, v, do)):
        assert torch.equal(g, t)
    outs = [guarded(q.shape, torch.float16), guarded(q.shape[:3], torch.float32)] + [guarded(q.shape, torch.float16) for _ in range(3)]
    outs += [guarded(q.shape[:3], torch.float32)] + ([guarded(q.shape, torch.float16)] if causal else [])  # O LSE dQ dK dV delta (O_causal)
    for buf, mid in outs:
        assert bool(torch.isfinite(buf[0]).all()) and bool(torch.isfinite(buf[-1]).all()) and bool(torch.isnan(mid).all())
    saved = [pads(buf) for buf, _ in outs]
    (_, go), (_, gl), (_, gdq), (_, gdk), (_, gdv), (_, gdl) = outs[:6]
    gq, gk, gv, gdo = ins
    fwd_lse(gq, gk, gv, causal, o=go, lse=gl)
    if causal:
        fwd_causal(gq, gk, gv, o=outs[6][1])
    # the O of the guarded run feeds the backward, itself between NaN pads
    bwd(gq, gk, gv, go, gdo, gl, causal, outs=(gdq, gdk, gdv, gdl))
    names = OUT_NAMES + ("O_causal",)
    for name, (buf, mid), keep, want in zip(names, outs, saved, plain):
        assert torch.equal(pads(buf), keep), (what, name, "pad overwritten")
        assert bool(torch.isfinite(mid).all()), (what, name)
        assert torch.equal(mid, want), (what, name, "payload differs from the run on ordinary allocations")
    # stages = 1 of the forward, guarded as well
    go.fill_(float("nan"))
    gl.fill_(float("nan"))
    fwd_lse(gq, gk, gv, causal, stages=1, o=go, lse=gl)
    assert torch.equal(pads(outs[0][0]), saved[0]) and torch.equal(pads(outs[1][0]), saved[1]), what
    assert torch.equal(go, plain[0]) and torch.equal(gl, plain[1]), what
    print("%-58s pads intact, payloads bit-identical" % what)


# ---- d. causality of the backward, bit-exact


def replaced(t, sl, amp, g):
    t2 = t.clone()
    t2[:, :, sl] = (torch.randn(t2[:, :, sl].shape, generator=g) * amp).half().cuda()
    return t2


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("cut", [127, 255, 300, 511])  # tile / row-block edges and inside a diagonal tile
def test_backward_ignores_future_keys(built, D, cut):
    q, k, v, do = gauss(1, 8, 1024, D, seed=8100 + D)
    base = run_all(q, k, v, do, True)
    g = torch.Generator().manual_seed(99)
    for amp in (1.0, 100.0):
        k2, v2 = replaced(k, slice(cut + 1, None), amp, g), replaced(v, slice(cut + 1, None), amp, g)
        assert not torch.equal(k2, k) and torch.equal(k2[:, :, :cut + 1], k[:, :, :cut + 1])
        new = run_all(q, k2, v2, do, True)
        for name, a, b in zip(OUT_NAMES, new, base):
            assert bool(torch.isfinite(a).all()), (name, amp, cut)
            if name in ("O", "LSE", "dQ", "delta"):
                assert torch.equal(a[:, :, :cut + 1], b[:, :, :cut + 1]), (name, amp, cut)
        assert not torch.equal(new[2][:, :, cut + 1:], base[2][:, :, cut + 1:])  # the replacement did reach the later rows


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("cut", [127, 255, 300, 511])
def test_backward_ignores_past_queries(built, D, cut):
    q, k, v, do = gauss(1, 8, 1024, D, seed=8200 + D)
    base = run_all(q, k, v, do, True)
    g = torch.Generator().manual_seed(98)
    for amp in (1.0, 100.0):
        q2, do2 = replaced(q, slice(0, cut), amp, g), replaced(do, slice(0, cut), amp, g)
        assert not torch.equal(q2, q) and torch.equal(q2[:, :, cut:], q[:, :, cut:])
        new = run_all(q2, k, v, do2, True)
        for name, a, b in zip(OUT_NAMES, new, base):
            assert bool(torch.isfinite(a).all()), (name, amp, cut)
            assert torch.equal(a[:, :, cut:], b[:, :, cut:]), (name, amp, cut)  # (delta too: rowsum of the row's own dO and O)
        assert not torch.equal(new[3][:, :, :cut], base[3][:, :, :cut])  # dK of the earlier keys did change


# ---- e. head independence, bit-exact


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("BH", [(2, 3), (1, 8)])
def test_heads_are_independent(built, causal, D, BH):
    N, n = 512, BH[0] * BH[1]
    ins = gauss(*BH, N, D, seed=8300 + D + n + int(causal))
    base = run_all(*ins, causal) + ((fwd_causal(*ins[:3]),) if causal else ())
    g = torch.Generator().manual_seed(97)
    for h in (0, n // 2, n - 1):
        what = "heads N=%d D=%d causal=%d BH=%s head %d" % (N, D, causal, BH, h)
        ins2 = [t.clone() for t in ins]
        for t in ins2:
            t.view(n, N, D)[h] = torch.randn(N, D, generator=g).half().cuda()
        new = run_all(*ins2, causal) + ((fwd_causal(*ins2[:3]),) if causal else ())
        others = [i for i in range(n) if i != h]
        for name, a, b in zip(OUT_NAMES + ("O_causal",), new, base):
            fa, fb = a.reshape(n, N, -1), b.reshape(n, N, -1)
            assert torch.equal(fa[others], fb[others]), (what, name)
            assert not torch.equal(fa[h], fb[h]), (what, name)
        check_case(what, *ins2, causal, heads=[h], outs=new[:6])


# ---- f. one-hot attention: exact answers, scores of 120-170 nats


def fp16_ulp(x):
    return torch.finfo(torch.float16).eps * torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14))))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,D", [(768, 64), (4096, 64), (768, 128), (4096, 128)])
def test_onehot_attention(built, causal, N, D):
    what = "onehot N=%d D=%d causal=%d" % (N, D, causal)
    H = 8
    heads = [far.onehot_problem(N, D, causal, seed=9000 + 16 * N + D + 8 * int(causal) + h) for h in range(H)]
    q, k, v, do = (torch.stack([hd[i] for hd in heads])[None].cuda() for i in range(4))
    pi = torch.stack([hd[4] for hd in heads])  # [H, N]
    o, lse, dq, dk, dv, delta = run_all(q, k, v, do, causal)
    outs = {"O": o, "LSE": lse, "dQ": dq, "dK": dk, "dV": dv, "delta": delta, "O_st1": fwd_lse(q, k, v, causal, stages=1)[0]}
    if causal:
        outs["O_caus"] = fwd_causal(q, k, v)
    for name, t in outs.items():
        assert bool(torch.isfinite(t).all()), (what, name)
    l64, o64, dq64, dk64, dv64 = far.ref_chunked(q, k, v, do, causal)
    idx = pi[:, :, None].expand(H, N, D)
    vd, dd, kd = (t[0].double().cpu() for t in (v, do, k))
    s_true = (q[0].double().cpu() * kd.gather(1, idx)).sum(-1) / D ** 0.5
    print("%-58s off-target mass %.3e, target score %.1f nats, gap %.1f nats" % (
        what, (-torch.expm1(s_true - l64)).max().item(), s_true.max().item(), 2 * 16 * (D // (N - 1).bit_length()) / D ** 0.5))
    # O = V[pi]: one fp16 rounding plus the off-target mass (<= 2.5e-8, tests/test_fa_reference.py) times max|V|
    vp = vd.gather(1, idx)
    for name in ("O", "O_st1", "O_caus"):
        if name in outs:
            diff, bound = (far.flat(outs[name]) - vp).abs(), 2.0 ** -10 * vp.abs() + 1e-5
            report(what, name, diff.max().item(), bound[diff == diff.max()].max().item())
            assert bool((diff <= bound).all()), (what, name, (diff - bound).max().item())
            assert maxerr(far.flat(outs[name]), o64) <= far.fa_tol(o64), (what, name)
    # LSE_i = s(i, pi(i)), the score as the kernel forms it from its pre-scaled Q
    sc = torch.tensor(far.LOG2E / D ** 0.5, dtype=torch.half)
    s_k = ((q[0].cpu() * sc).double() * kd.gather(1, idx)).sum(-1) / far.LOG2E
    report(what, "LSE", maxerr(far.flat(lse), s_k), 1e-5 * max(1.0, s_k.abs().max().item()))
    assert maxerr(far.flat(lse), s_k) <= 1e-5 * max(1.0, s_k.abs().max().item()), what
    # dV = index_add(pi, dO): not causal, a pure permutation of the rows of dO
    want = torch.zeros(H, N, D, dtype=torch.float64).scatter_add_(1, idx, dd)
    bound = 2.0 ** -10 * torch.zeros(H, N, D, dtype=torch.float64).scatter_add_(1, idx, dd.abs()) + 1e-5
    diff = (far.flat(dv) - want).abs()
    report(what, "dV", diff.max().item(), bound[diff == diff.max()].max().item())
    assert bool((diff <= bound).all()), (what, "dV", (diff - bound).max().item())
    # dQ, dK: ~0 in truth; the kernel's values are fp32 noise in dP - delta
    gb = 2.0 ** -9 * dv64.abs().max().item()
    for name, x, x64 in (("dQ", dq, dq64), ("dK", dk, dk64)):
        report(what, name, maxerr(far.flat(x), x64), gb)
        assert maxerr(far.flat(x), x64) <= gb, (what, name)
    check_delta(delta, do, o, what)


# ---- g. closed forms and scaled dO


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_zero_queries(built, causal, D):
    N = 1024
    what = "Q=0 D=%d causal=%d" % (D, causal)
    _, k, v, do = gauss(1, 8, N, D, seed=9100 + D + int(causal))
    q = torch.zeros_like(k)
    o, lse, dq, dk, dv, delta = run_all(q, k, v, do, causal)
    vd = far.flat(v)
    cnt = torch.arange(1, N + 1, dtype=torch.float64)
    l_ref = cnt.log().expand(8, N) if causal else torch.full((8, N), math.log(N), dtype=torch.float64)
    o_ref = vd.cumsum(1) / cnt[None, :, None] if causal else vd.mean(1, keepdim=True).expand(8, N, D)
    report(what, "LSE", maxerr(far.flat(lse), l_ref), 1e-5 * max(1.0, math.log(N)))
    assert maxerr(far.flat(lse), l_ref) <= 1e-5 * max(1.0, math.log(N)), what
    outs = [("O", o), ("O_st1", fwd_lse(q, k, v, causal, stages=1)[0])] + ([("O_caus", fwd_causal(q, k, v))] if causal else [])
    for name, t in outs:
        report(what, name, maxerr(far.flat(t), o_ref), far.fa_tol(o_ref))
        assert maxerr(far.flat(t), o_ref) <= far.fa_tol(o_ref), (what, name)
    assert torch.equal(dk, torch.zeros_like(dk)), (what, dk.abs().max().item())
    check_case(what, q, k, v, do, causal, outs=(o, lse, dq, dk, dv, delta))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_constant_values(built, causal, D):
    """V the same row for every key: whatever P is, O = (sum_j P_j / l) V_0, so a normaliser l that disagrees with the fp16 P the kernel
    multiplies by V shows as more than the one rounding of the result."""
    N = 1024
    q, k, _, _ = gauss(1, 8, N, D, seed=9200 + D + int(causal))
    v0 = torch.randn(1, 8, 1, D, generator=torch.Generator().manual_seed(9300 + D)).half().cuda()
    v = v0.expand(1, 8, N, D).contiguous()
    outs = [("O", fwd_lse(q, k, v, causal)[0]), ("O_st1", fwd_lse(q, k, v, causal, stages=1)[0])]
    outs += [("O_caus", fwd_causal(q, k, v))] if causal else []
    for name, o in outs:
        diff = (o.float() - v.float()).abs()
        ulps = (diff / fp16_ulp(v.float())).max().item()
        report("constant V D=%d causal=%d" % (D, causal), name, ulps, 1.0)
        assert bool((diff <= fp16_ulp(v.float())).all()), (name, ulps)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_key_gradients_sum_to_zero(built, causal, D):
    """Softmax shift invariance: sum_j dK_j = 0. The fp16 rounding of the N outputs alone allows 2^-11 sum_j |dK64_j| per element (each
    |error| <= 2^-11 |dK_j|); the test allows twice that for everything before the rounding."""
    N = 1024
    what = "sum_j dK_j D=%d causal=%d" % (D, causal)
    q, k, v, do = gauss(1, 8, N, D, seed=9400 + D + int(causal))
    dk = run_all(q, k, v, do, causal)[3]
    dk64 = far.ref_chunked(q, k, v, do, causal)[3]
    allowed = 2.0 ** -11 * dk64.abs().sum(1)
    assert bool((dk64.half().double().sum(1).abs() <= allowed).all())  # the rounded reference meets the bound it sets
    got = far.flat(dk).sum(1).abs()
    worst = (got / (2 * allowed)).argmax()
    report(what, "sum dK", got.flatten()[worst].item(), 2 * allowed.flatten()[worst].item())
    assert bool((got <= 2 * allowed).all()), (what, (got / (2 * allowed)).max().item())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("exp", [6, -6])
def test_scaled_output_gradient(built, causal, D, exp):
    """dO * 2^6 / 2^-6 (loss scaling): the gradient rule against the reference and SDPA's fp16 gradients of the same scaled dO."""
    q, k, v, do = gauss(1, 8, 1024, D, seed=9500 + D + int(causal))
    do = (do.float() * 2.0 ** exp).half()
    check_case("dO * 2^%d D=%d causal=%d" % (exp, D, causal), q, k, v, do, causal)
