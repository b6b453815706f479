"""GPU: single-query attention over a KV cache (cuda_learn_notes_amd.fa2_decode, cln_fa2_decode; csrc/flash_attn_decode.cuh) against the fp64
reference of tests/decode_reference.py: parity at the plan's own boundaries, nothing past the length is read, guard bands around every output,
answers known exactly, independence of the neighbours, repeatability, agreement with the causal prefill kernel, graph replay with lengths changed
on the device, and the Python argument errors. Every case prints its figures before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
from fa_reference import onehot_problem  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, H, Nmax): chosen from the plan (decode_reference.plan mirrors it; test_shapes_cover_one_split_and_many asserts what they cover)
SHAPES = [(1, 1, 8192), (2, 8, 4096), (3, 5, 1000), (2, 8, 200), (3, 5, 63), (1, 1, 1)]
DS = [64, 128]


@functools.lru_cache(maxsize=None)
def problem(B, H, Nmax, D, seed=0):
    """Gaussian fp16 (q, k, v) on the CPU, made once per shape and never modified."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * H + Nmax + D)
    q = torch.randn(B, H, D, generator=g).half()
    k, v = (torch.randn(B, H, Nmax, D, generator=g).half() for _ in range(2))
    return q, k, v


def lengths_for(B, H, Nmax, D):
    S, C, _ = dr.plan(B, H, Nmax, D)
    step = dr.key_step(D)
    want = [1, 2, step - 1, step, step + 1, C - 1, C, C + 1, 2 * C + 1, Nmax - 1, Nmax]
    return sorted({n for n in want if 1 <= n <= Nmax})


def run(q, k, v, lens, want_lse=True, workspace=None, dev="cuda"):
    import cuda_learn_notes_amd as pkg
    qd, kd, vd = (t.to(dev) if not t.is_cuda else t for t in (q, k, v))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full_like(qd, float("nan"))
    lse = torch.full(qd.shape[:2], float("nan"), dtype=torch.float32, device=dev) if want_lse else None
    pkg.fa2_decode(qd, kd, vd, sl, o, lse, workspace)
    torch.cuda.synchronize()
    return o.cpu(), (lse.cpu() if want_lse else None)


def check(o, lse, q, k, v, lens, what):
    """O within fa_tol(ref), LSE within 2^-10 max(1, max|LSE_ref|); returns the two ratios error / bound."""
    ro, rl = dr.ref_decode(q, k, v, lens)
    assert bool(torch.isfinite(o).all()), what
    eo, bo = (o.double() - ro).abs().max().item(), dr.fa_tol(ro)
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float("-inf")).all()), what
    el = (lse.double()[fin] - rl[fin]).abs().max().item() if bool(fin.any()) else 0.0
    bl = dr.lse_tol(rl)
    print("%s: O err %.3e / bound %.3e = %.4f   LSE err %.3e / bound %.3e = %.4f" % (what, eo, bo, eo / bo, el, bl, el / bl))
    assert eo <= bo, (what, eo, bo)
    assert el <= bl, (what, el, bl)
    return eo / bo, el / bl


def test_shapes_cover_one_split_and_many(built):
    for D in DS:
        splits = [built.fa2_decode_plan(B, H, Nmax, D)[0] for (B, H, Nmax) in SHAPES]
        assert splits == [dr.plan(B, H, Nmax, D)[0] for (B, H, Nmax) in SHAPES]
        assert any(s == 1 for s in splits) and any(s >= 3 for s in splits), (D, splits)
    assert {(B, H) for (B, H, _) in SHAPES} == {(1, 1), (2, 8), (3, 5)} and max(n for (_, _, n) in SHAPES) <= 8192
    assert {1, 63, 1000} <= {n for (_, _, n) in SHAPES}


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_at_the_plan_boundaries(built, dev, shape, D):
    B, H, Nmax = shape
    q, k, v = problem(B, H, Nmax, D)
    qd, kd, vd = (t.to(dev) for t in (q, k, v))
    worst = (0.0, 0.0)
    for n in lengths_for(B, H, Nmax, D):
        o, lse = run(qd, kd, vd, [n] * B)
        r = check(o, lse, q, k, v, [n] * B, "D=%d %s len=%d" % (D, shape, n))
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("D=%d %s S=%d C=%d: worst error / bound  O %.4f  LSE %.4f" % ((D, shape) + dr.plan(B, H, Nmax, D)[:2] + worst))


@pytest.mark.parametrize("D", DS)
def test_mixed_batch(built, dev, D):
    """A length of 1, a length that leaves the last S - 1 splits empty, and Nmax, in one batch."""
    B, H, Nmax = 3, 5, 1000
    S, C, _ = dr.plan(B, H, Nmax, D)
    assert S >= 3 and C - 3 > 1
    lens = [1, C - 3, Nmax]
    q, k, v = problem(B, H, Nmax, D)
    o, lse = run(q, k, v, lens)
    check(o, lse, q, k, v, lens, "D=%d %s lens=%s" % (D, (B, H, Nmax), lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 8, 4096), (3, 5, 1000), (2, 8, 200)], ids=lambda s: "x".join(map(str, s)))
def test_nothing_past_the_length_is_used(built, dev, shape, D):
    B, H, Nmax = shape
    S, C, need = dr.plan(B, H, Nmax, D)
    q, k, v = problem(B, H, Nmax, D)
    lens = [C + 1, Nmax - 1, 5][:B]
    outs = []
    for fill in (float("nan"), 6e4):
        kf, vf = k.clone(), v.clone()
        for b in range(B):
            kf[b, :, lens[b]:] = fill
            vf[b, :, lens[b]:] = fill
        ws = torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device=dev)
        outs.append(run(q, kf, vf, lens, workspace=ws))
    plain = run(q, k, v, lens)
    for o, lse in outs:
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
        assert torch.equal(o, plain[0]) and torch.equal(lse, plain[1])
    check(plain[0], plain[1], q, k, v, lens, "D=%d %s lens=%s" % (D, shape, lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 8, 4096), (3, 5, 1000), (3, 5, 63)], ids=lambda s: "x".join(map(str, s)))
def test_guard_bands(built, dev, shape, D):
    import cuda_learn_notes_amd as pkg
    B, H, Nmax = shape
    S, C, need = pkg.fa2_decode_plan(B, H, Nmax, D)
    q, k, v = (t.to(dev) for t in problem(B, H, Nmax, D))
    G = 256
    ob = torch.full((B * H * D + 2 * G,), 777.0, dtype=torch.half, device=dev)
    lb = torch.full((B * H + 2 * G,), 777.0, dtype=torch.float32, device=dev)
    wb = torch.full((need + 2 * G,), 0xA5, dtype=torch.uint8, device=dev)
    o, lse, ws = ob[G:G + B * H * D].view(B, H, D), lb[G:G + B * H].view(B, H), wb[G:G + need]
    assert ws.numel() == need
    lens = torch.tensor([Nmax, 1, Nmax // 2][:B], dtype=torch.int32, device=dev)
    pkg.fa2_decode(q, k, v, lens, o, lse, ws if need else None)
    torch.cuda.synchronize()
    for buf, n in ((ob, B * H * D), (lb, B * H)):
        assert bool((buf[:G] == 777.0).all()) and bool((buf[G + n:] == 777.0).all())
    assert bool((wb[:G] == 0xA5).all()) and bool((wb[G + need:] == 0xA5).all())
    check(o.cpu(), lse.cpu(), *problem(B, H, Nmax, D), lens.tolist(), "guarded D=%d %s" % (D, shape))


@pytest.mark.parametrize("D", DS)
def test_one_hot_keys_select_one_value_row(built, dev, D):
    N = 4096  # (1, 1, 4096): the plan splits the keys 16 ways
    assert dr.plan(1, 1, N, D)[0] >= 3
    _, k, v, _, _ = onehot_problem(N, D, False, seed=5)
    bits = (N - 1).bit_length()
    score = 16.0 * (D // bits) * bits / D ** 0.5
    for n, t in ((N, 0), (N, N - 1), (3000, 2999), (3000, 1234), (257, 256)):
        q = (k[t] * 16).view(1, 1, D)
        o, lse = run(q, k.view(1, 1, N, D), v.view(1, 1, N, D), [n])
        assert torch.equal(o.view(D), v[t]), (D, n, t)
        assert abs(lse.item() - score) <= 1e-5 * score, (D, n, t, lse.item(), score)


@pytest.mark.parametrize("D", DS)
def test_constant_values_zero_query_and_single_key(built, dev, D):
    B, H, Nmax = 3, 5, 1000
    q, k, v = problem(B, H, Nmax, D)
    lens = [1000, 385, 77]
    # constant V: every accumulator sums at most a few dozen terms c p in fp32, relative error ~1e-6, far below half an fp16 ulp of c
    o, _ = run(q, k, torch.full_like(v, 0.375), lens)
    assert bool((o == 0.375).all())
    # q = 0: the mean of the live rows, LSE = ln(len)
    z = torch.zeros_like(q)
    o, lse = run(z, k, v, lens)
    for b in range(B):
        mean = v[b, :, :lens[b]].double().mean(dim=1)
        assert (o[b].double() - mean).abs().max().item() <= dr.fa_tol(mean), (D, b)
        ln = torch.log(torch.tensor(float(lens[b]), dtype=torch.float64)).item()
        assert (lse[b].double() - ln).abs().max().item() <= 1e-6 * ln, (D, b, lse[b], ln)
    # one key: O = V[0] bit for bit; LSE = q . K_0 / sqrt(D), an fp32 dot product of D exact products (error <= (D + 4) 2^-24 sum|q_i k_i| / sqrt(D))
    o, lse = run(q, k, v, [1] * B)
    assert torch.equal(o, v[:, :, 0])
    s = (q.double() * k[:, :, 0].double()).sum(-1) / D ** 0.5
    bound = (D + 4) * 2.0 ** -24 * (q.double() * k[:, :, 0].double()).abs().sum(-1) / D ** 0.5
    assert bool(((lse.double() - s).abs() <= bound).all()), (D, (lse.double() - s).abs().max().item(), bound.min().item())


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 5, 1000), (2, 8, 200)], ids=lambda s: "x".join(map(str, s)))
def test_lengths_are_clamped(built, dev, shape, D):
    B, H, Nmax = shape
    q, k, v = problem(B, H, Nmax, D)
    o, lse = run(q, k, v, [0, -3, 0][:B])
    assert bool((o == 0).all()) and bool((lse == float("-inf")).all())
    full = run(q, k, v, [Nmax] * B)
    over = run(q, k, v, [Nmax + 7] * B)
    assert torch.equal(full[0], over[0]) and torch.equal(full[1], over[1])
    mixed = run(q, k, v, [0, Nmax + 7, -3][:B])
    assert bool((mixed[0][0] == 0).all()) and torch.equal(mixed[0][1], full[0][1]) and torch.equal(mixed[1][1], full[1][1])
    assert mixed[1][0].tolist() == [float("-inf")] * H


@pytest.mark.parametrize("D", DS)
def test_a_sequence_does_not_depend_on_its_neighbours_and_calls_repeat(built, dev, D):
    B, H, Nmax = 3, 5, 1000
    q, k, v = problem(B, H, Nmax, D)
    first = run(q, k, v, [700, 999, 333])
    k2, v2 = problem(B, H, Nmax, D, seed=1)[1:]
    k2, v2 = k2.clone(), v2.clone()
    k2[1], v2[1] = k[1], v[1]
    other = run(q, k2, v2, [1, 999, 1000])
    assert torch.equal(first[0][1], other[0][1]) and torch.equal(first[1][1], other[1][1])
    assert not torch.equal(first[0][0], other[0][0])
    import cuda_learn_notes_amd as pkg
    qd, kd, vd = (t.to(dev) for t in (q, k, v))
    sl = torch.tensor([700, 999, 333], dtype=torch.int32, device=dev)
    ws = torch.empty(max(pkg.fa2_decode_plan(B, H, Nmax, D)[2], 16), dtype=torch.uint8, device=dev)
    outs = [(torch.empty_like(qd), torch.empty(B, H, dtype=torch.float32, device=dev)) for _ in range(20)]
    for o, l in outs:
        pkg.fa2_decode(qd, kd, vd, sl, o, l, ws)
    torch.cuda.synchronize()
    assert all(torch.equal(o.cpu(), first[0]) and torch.equal(l.cpu(), first[1]) for o, l in outs)


@pytest.mark.parametrize("D", DS)
def test_agrees_with_the_last_row_of_the_causal_prefill(built, dev, D):
    import cuda_learn_notes_amd as pkg
    B, H, N = 2, 8, 512
    g = torch.Generator().manual_seed(77 + D)
    Q, K, V = (torch.randn(B, H, N, D, generator=g).half() for _ in range(3))
    Qd, Kd, Vd = (t.to(dev) for t in (Q, K, V))
    O = torch.empty_like(Qd)
    pkg.fa2_fwd_causal(Qd, Kd, Vd, O)
    q = Q[:, :, N - 1].contiguous()
    o, _ = run(q, Kd, Vd, [N] * B)
    ref, _ = dr.ref_decode(q, K, V, [N] * B)
    err = (o.float() - O[:, :, N - 1].cpu().float()).abs().max().item()
    print("D=%d: decode vs causal prefill last row %.3e, bound %.3e" % (D, err, 2 * dr.fa_tol(ref)))
    assert err <= 2 * dr.fa_tol(ref)  # the prefill kernel carries its own fp16 pre-scaled Q error


@pytest.mark.parametrize("D", DS)
def test_graph_replay_reads_lengths_and_cache_from_the_device(built, dev, D):
    import cuda_learn_notes_amd as pkg
    B, H, Nmax = 2, 8, 4096
    S, C, need = pkg.fa2_decode_plan(B, H, Nmax, D)
    assert S > 1  # two kernels in a line
    q, k, v = (t.to(dev).clone() for t in problem(B, H, Nmax, D))
    sl = torch.tensor([100, 4096], dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    og, lg = torch.zeros_like(q), torch.zeros(B, H, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pkg.fa2_decode(q, k, v, sl, og, lg, ws)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pkg.fa2_decode(q, k, v, sl, og, lg, ws)
    sl.copy_(torch.tensor([3000, 513], dtype=torch.int32, device=dev))
    k[0, 3, 2999] = torch.randn(D, device=dev).half() * 4
    og.zero_(), lg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    oe, le = torch.empty_like(q), torch.empty_like(lg)
    pkg.fa2_decode(q, k, v, sl, oe, le)
    torch.cuda.synchronize()
    assert torch.equal(og, oe) and torch.equal(lg, le)
    check(og.cpu(), lg.cpu(), q.cpu(), k.cpu(), v.cpu(), [3000, 513], "graph replay D=%d" % D)


def test_python_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    B, H, Nmax, D = 2, 8, 4096, 64
    q, k, v = (t.to(dev) for t in problem(B, H, Nmax, D))
    sl = torch.tensor([5, 9], dtype=torch.int32, device=dev)
    o = torch.empty_like(q)
    need = pkg.fa2_decode_plan(B, H, Nmax, D)[2]
    assert need > 0
    bad = [
        lambda: pkg.fa2_decode(q.float(), k, v, sl, o),                                      # dtype
        lambda: pkg.fa2_decode(q, k, v, sl.long(), o),
        lambda: pkg.fa2_decode(q, k, v, sl, o, lse=torch.empty(B, H, dtype=torch.half, device=dev)),
        lambda: pkg.fa2_decode(q, k[:, :, :100].contiguous(), v, sl, o),                     # shape
        lambda: pkg.fa2_decode(q, k, v, sl[:1], o),
        lambda: pkg.fa2_decode(q, k, v, sl, o[:, :4].contiguous()),
        lambda: pkg.fa2_decode(q, k, v, sl, o, lse=torch.empty(B, H + 1, dtype=torch.float32, device=dev)),
        lambda: pkg.fa2_decode(q.unsqueeze(2), k, v, sl, o),
        lambda: pkg.fa2_decode(q, k, v, sl.cpu(), o),                                        # seqlens on the CPU
        lambda: pkg.fa2_decode(q, k, v, sl, o, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev)),  # short workspace
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
        print("argument error %d raised" % i)
    q96, k96 = torch.zeros(1, 2, 96, dtype=torch.half, device=dev), torch.zeros(1, 2, 64, 96, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="headdim 96"):
        pkg.fa2_decode(q96, k96, k96.clone(), sl[:1], torch.empty_like(q96))
