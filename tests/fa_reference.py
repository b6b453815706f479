"""fp64 CPU references for the attention tests (tests/test_fa_reference.py proves them, tests/test_gpu_fa2_edges.py uses them): the
closed-form forward and backward of softmax(Q K^T / sqrt(D)) V in chunks of query rows (no autograd, O(chunk N) memory, so N = 16384 is
affordable), the log-sum-exp of the scores the kernels form from their fp16 pre-scaled Q, a one-hot problem whose answers are known
exactly, and the tolerance rules of tests/test_gpu_fa2_causal.py / tests/test_gpu_fa2_bwd.py. A plain module: nothing here is collected."""
import torch

LOG2E = 1.4426950408889634
TOL_AMPLIFIED_KEYS = 6e-3


def _heads(t, heads):
    B, H = t.shape[:2]
    return list(range(B * H)) if heads is None else list(heads)


def ref_chunked(q, k, v, do, causal, heads=None, chunk=1024):
    """fp64 (lse, O, dQ, dK, dV) of softmax(Q K^T / sqrt(D), masked to key <= query when causal) V per flattened head, each
    [len(heads), N(, D)]. For a chunk of query rows [r0, r1): S, lse = logsumexp(S), P = exp(S - lse), O = P V, dP = dO V^T,
    delta = rowsum(dO o O), dS = P o (dP - delta) / sqrt(D), dQ = dS K, dK += dS^T Q, dV += P^T dO. A causal chunk only touches keys < r1."""
    B, H, N, D = q.shape
    hs = _heads(q, heads)
    qf, kf, vf, df = (t.reshape(B * H, N, D)[hs].double().cpu() for t in (q, k, v, do))
    lse = torch.empty(len(hs), N, dtype=torch.float64)
    o, dq, dk, dv = torch.empty_like(qf), torch.empty_like(qf), torch.zeros_like(qf), torch.zeros_like(qf)
    rs = 1.0 / D ** 0.5
    for h in range(len(hs)):
        for r0 in range(0, N, chunk):
            r1 = min(r0 + chunk, N)
            nk = r1 if causal else N
            qc, dc, kc, vc = qf[h, r0:r1], df[h, r0:r1], kf[h, :nk], vf[h, :nk]
            s = qc @ kc.T * rs
            if causal:
                s.masked_fill_(torch.arange(nk)[None, :] > torch.arange(r0, r1)[:, None], float("-inf"))
            l = torch.logsumexp(s, dim=-1)
            p = torch.exp(s - l[:, None])
            oc = p @ vc
            ds = p * (dc @ vc.T - (dc * oc).sum(-1, keepdim=True)) * rs
            lse[h, r0:r1], o[h, r0:r1], dq[h, r0:r1] = l, oc, ds @ kc
            dk[h, :nk] += ds.T @ qc
            dv[h, :nk] += p.T @ dc
    return lse, o, dq, dk, dv


def kernel_scores_lse(q, k, causal, heads=None, chunk=1024):
    """fp64 logsumexp, [len(heads), N], of the scores the kernels form: fp16(Q * fp16(log2 e / sqrt D)) . K, times ln 2 (the second
    reference of check_lse), in chunks of query rows."""
    B, H, N, D = q.shape
    hs = _heads(q, heads)
    sc = torch.tensor(LOG2E / D ** 0.5, dtype=torch.half)
    qs = (q.reshape(B * H, N, D)[hs].cpu() * sc).double()
    kf = k.reshape(B * H, N, D)[hs].double().cpu()
    out = torch.empty(len(hs), N, dtype=torch.float64)
    for r0 in range(0, N, chunk):
        r1 = min(r0 + chunk, N)
        nk = r1 if causal else N
        s = qs[:, r0:r1] @ kf[:, :nk].transpose(-1, -2) / LOG2E
        if causal:
            s = s.masked_fill(torch.arange(nk)[None, :] > torch.arange(r0, r1)[:, None], float("-inf"))
        out[:, r0:r1] = torch.logsumexp(s, dim=-1)
    return out


def onehot_problem(N, D, causal, seed):
    """(q, k, v, do, pi), fp16 [N, D] and int64 [N], of one head whose softmax is one-hot to ~1e-8: key j is the +-1 binary code of j over
    bits = (N - 1).bit_length() dimensions, repeated r = D // bits times (the rest 0); q_i = 16 k_pi(i) with pi a seeded permutation
    (causal: a seeded map with pi(i) <= i); v, do ~ N(0, 1). Every entry is exact in fp16 and so is every score the kernels form
    (16 log2 e / sqrt D rounds once, the products are integers times it). Row i scores 16 r bits / sqrt(D) on key pi(i) and at most
    that minus 2 * 16 r / sqrt(D) nats elsewhere (one code bit differs): >= 20 nats for N <= 4096 at D = 64, >= 28 at D = 128. Then
    O = V[pi], LSE_i = s(i, pi(i)) and dV = index_add(pi, dO) up to that off-target mass, and dQ, dK ~ 0. Not for N > 4096 at D = 64
    (N = 16384: 16 nats, mass 1.6e-6)."""
    bits = (N - 1).bit_length()
    r = D // bits
    assert r >= 1 and 2 * 16 * r / D ** 0.5 >= 20.0, (N, D)
    g = torch.Generator().manual_seed(seed)
    code = ((torch.arange(N)[:, None] >> torch.arange(bits)[None, :]) & 1) * 2 - 1
    k = torch.zeros(N, D, dtype=torch.half)
    k[:, :r * bits] = code.repeat(1, r).half()
    if causal:
        pi = (torch.rand(N, generator=g, dtype=torch.float64) * torch.arange(1, N + 1)).floor().long()
        pi = torch.minimum(pi, torch.arange(N))
    else:
        pi = torch.randperm(N, generator=g)
    q = k[pi] * 16
    v, do = (torch.randn(N, D, generator=g).half() for _ in range(2))
    return q, k, v, do, pi


# ---- the tolerance rules of tests/test_gpu_fa2_causal.py (fa_tol), tests/test_gpu_flash_attn.py (fa_tol_f32) and tests/test_gpu_fa2_bwd.py
# (check_grads, check_lse, flat), copied


def fa_tol(ref):
    """The scale rule of the plain attention names: 2^-9 max|O_ref| + 4e-4, never more than the amplified-key bound 6e-3."""
    return min(2.0 ** -9 * float(ref.abs().max()) + 4e-4, TOL_AMPLIFIED_KEYS)


TOL_F32_CAP = 3e-3


def fa_tol_f32(ref):
    """The same for the kernels that scale the scores in fp32 (the *_acc_f32 names, the split-KV rung, every name at D >= 256): 2^-10 max|O_ref| + 2e-4,
    never more than 3e-3 (the flat bound of rounds 1-5). Measured worst case / bound: 0.56 (N(0,1): 7.2e-4 at D = 512; keys x4: 2.3e-3 at max|O| = 4)."""
    return min(2.0 ** -10 * float(ref.abs().max()) + 2e-4, TOL_F32_CAP)


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


# ---- guard bands (tests/test_gpu_fa2_edges.py, tests/test_gpu_fa2_plain_edges.py): every tensor is batches 1..B of a [B + 2, ...] buffer;
# input pads NaN, output pads a finite sentinel

SENTINEL = {torch.float16: (torch.int16, 0x3A5C), torch.float32: (torch.int32, 0x3F4B5A69)}  # 0.7949 / 0.7943: finite, unlikely results


def guarded(shape, dtype, payload=None):
    """(buffer, its middle slice). payload given: an input (pads NaN); None: an output (pads the sentinel, the slice NaN)."""
    B = shape[0]
    buf = torch.empty((B + 2,) + tuple(shape[1:]), dtype=dtype, device="cuda")
    mid = buf[1:B + 1]
    if payload is not None:
        buf.fill_(float("nan"))
        mid.copy_(payload)
    else:
        it, bits = SENTINEL[dtype]
        buf.view(it).fill_(bits)
        mid.fill_(float("nan"))
    assert mid.is_contiguous() and mid.data_ptr() % 16 == 0 and mid.data_ptr() > buf.data_ptr()
    return buf, mid


def pads(buf):
    it = SENTINEL[buf.dtype][0]
    return torch.stack((buf[0].view(it), buf[-1].view(it))).clone()
