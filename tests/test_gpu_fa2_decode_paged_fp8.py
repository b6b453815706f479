"""GPU: decode attention over a paged KV cache held in FP8 (cuda_learn_notes_amd.fa2_decode_paged_fp8, cln_fa2_decode_paged_fp8;
csrc/flash_attn_decode_paged_fp8.cuh) against the fp64 reference of tests/fp8_kv_reference.py ON THE DEQUANTISED POOLS: the kernel's error
against it is that of the fp16 kernel (fp32 accumulation, one fp16 rounding of O), so the bounds are decode_reference.fa_tol / lse_tol unchanged.
What quantising the cache costs is a property of the data; it is printed against the un-quantised fp64 answer and not asserted. Every case runs
on a pool with more pages than it needs, the live pages placed by a seeded permutation with the sequences interleaved, every page no live entry
names filled with the e4m3 NaN byte 0x7f and every table entry past ceil(len / page) pointing at an in-range poison page of it
(fp8_kv_reference.make_pool): a kernel that follows a wrong entry or reads a row too many gives NaN, not a fault. Every case prints its figures
before it asserts (pytest -s)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import fp8_kv_reference as f8  # noqa: E402
import kv_append_reference as kr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
from fa_reference import onehot_problem  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, Hkv, G, page, max_pages): the six shapes of tests/test_gpu_fa2_decode_paged.py; the plan of the FP8 entry still splits them 1 and >= 3 ways
# (test_shapes_cover_the_plan). Its key step is 256 at D = 64 and 128 at D = 128.
SHAPES = [(3, 2, 1, 16, 63), (2, 2, 4, 16, 64), (2, 1, 8, 128, 8), (1, 1, 2, 256, 32), (3, 5, 1, 32, 2), (1, 1, 8, 16, 1)]
DS = [64, 128]
ids = lambda s: "x".join(map(str, s))  # noqa: E731
bits = f8.bits


def plan_of(shape, D):
    B, Hkv, G, page, mp = shape
    return f8.plan(B, Hkv * G, Hkv, mp, page, D)


def scales_for(Hkv, which):
    """Per-head scales that differ across heads, near absmax / 448 of N(0, 1) data (absmax ~ 4.5)."""
    base = 0.0101 if which == "k" else 0.0093
    return torch.tensor([base * (1.0 + 0.37 * h) for h in range(Hkv)])


@functools.lru_cache(maxsize=None)
def problem(shape, D, seed=0):
    """On the CPU, made once per shape and never modified: q fp16 [B,Hq,D]; Gaussian dense k, v fp32 [B,Hkv,Nmax,D] and their e4m3 forms k8, v8
    under the per-head scales ks, vs."""
    B, Hkv, G, page, mp = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * Hkv + 17 * G + page * mp + D)
    q = torch.randn(B, Hkv * G, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, page * mp, D, generator=g) for _ in range(2))
    ks, vs = scales_for(Hkv, "k"), scales_for(Hkv, "v")
    return q, f8.quantize(k, f8.per_head(ks)), f8.quantize(v, f8.per_head(vs)), ks, vs, k, v


def lengths_for(shape, D):
    B, Hkv, G, page, mp = shape
    S, C, _ = plan_of(shape, D)
    step, Nmax = f8.key_step(D), page * mp
    want = [1, 2, page - 1, page, page + 1, step - 1, step, step + 1, C - 1, C, C + 1, 2 * C + 1, Nmax - 1, Nmax]
    return sorted({n for n in want if 1 <= n <= Nmax})


def run(q, kp, vp, bt, lens, ks, vs, want_lse=True, workspace=None, dev="cuda"):
    import cuda_learn_notes_amd as pkg
    qd, kd, vd, bd, ksd, vsd = (t.to(dev) if not t.is_cuda else t for t in (q, kp, vp, bt, ks, vs))
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    o = torch.full_like(qd, float("nan"))
    lse = torch.full(qd.shape[:2], float("nan"), dtype=torch.float32, device=dev) if want_lse else None
    pkg.fa2_decode_paged_fp8(qd, kd, vd, bd, sl, ksd, vsd, o, lse, workspace)
    torch.cuda.synchronize()
    return o.cpu(), (lse.cpu() if want_lse else None)


def check(o, lse, q, kp, vp, bt, lens, ks, vs, what):
    """O within fa_tol(ref), LSE within lse_tol(ref) of the reference on the dequantised pools; returns the two ratios error / bound."""
    ro, rl = f8.ref_decode_paged_fp8(q, kp, vp, ks, vs, bt, lens)
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


def pool_run_check(shape, D, lens, what, seed=0):
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    kp, vp, bt = f8.make_pool(k8, v8, shape[3], lens, seed=seed)
    o, lse = run(q, kp, vp, bt, lens, ks, vs)
    return (o, lse) + check(o, lse, q, kp, vp, bt, lens, ks, vs, what)


def test_shapes_cover_the_plan(built):
    for D in DS:
        step = f8.key_step(D)
        splits = [built.fa2_decode_paged_fp8_plan(B, Hkv * G, Hkv, mp, page, D)[0] for (B, Hkv, G, page, mp) in SHAPES]
        assert splits == [plan_of(s, D)[0] for s in SHAPES]
        assert any(s == 1 for s in splits) and any(s >= 3 for s in splits), (D, splits)
        assert {s[2] for s in SHAPES} == set(pr.GROUPS)
        assert any(s[3] < step for s in SHAPES), D
        # above the step: a page of 256 at D = 128 (step 128). At D = 64 the step is 256, the largest page there is: the page AT the step is the
        # boundary that exists (unit = max(page, step) takes either branch with the same value)
        assert any(s[3] > step for s in SHAPES) if D == 128 else any(s[3] == step for s in SHAPES), D
    assert any(s[3] < f8.key_step(D) for s in SHAPES for D in DS) and any(s[3] > f8.key_step(D) for s in SHAPES for D in DS)
    assert max(s[3] * s[4] for s in SHAPES) <= 8192


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parity_at_the_plan_boundaries(built, dev, shape, D):
    B = shape[0]
    worst = (0.0, 0.0)
    for i, n in enumerate(lengths_for(shape, D)):
        r = pool_run_check(shape, D, [n] * B, "D=%d %s len=%d" % (D, shape, n), seed=i)[2:]
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("D=%d %s S=%d C=%d: worst error / bound  O %.4f  LSE %.4f" % ((D, shape) + plan_of(shape, D)[:2] + worst))
    # what the cache format costs on this data, against the un-quantised fp64 answer: printed, not asserted
    q, k8, v8, ks, vs, k, v = problem(shape, D)
    Nmax = shape[3] * shape[4]
    G = shape[2]
    ro, _ = dr.ref_decode(q, k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1), [Nmax] * B)
    rq, _ = dr.ref_decode(q, f8.dequantize(k8, f8.per_head(ks)).repeat_interleave(G, dim=1),
                          f8.dequantize(v8, f8.per_head(vs)).repeat_interleave(G, dim=1), [Nmax] * B)
    print("D=%d %s: quantisation error of O at len %d: max %.3e (max|O| %.3e)" % (D, shape, Nmax, (rq - ro).abs().max().item(), ro.abs().max().item()))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 2, 1, 16, 64), (3, 1, 4, 32, 32)], ids=ids)
def test_mixed_batch(built, dev, shape, D):
    """A length of 1, a length that leaves the last S - 1 splits empty, and Nmax, in one batch."""
    S, C, _ = plan_of(shape, D)
    assert S >= 3 and C - 3 > 1
    lens = [1, C - 3, shape[3] * shape[4]]
    pool_run_check(shape, D, lens, "D=%d %s lens=%s" % (D, shape, lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (2, 1, 8, 128, 8)], ids=ids)
def test_page_placement_does_not_change_a_bit(built, dev, shape, D):
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    Nmax = shape[3] * shape[4]
    lens = [Nmax - 324, Nmax]
    pools = [f8.make_pool(k8, v8, shape[3], lens, **kw) for kw in (dict(order="identity"), dict(seed=1), dict(seed=2, extra=9))]
    assert not torch.equal(pools[0][2], pools[1][2]) and not torch.equal(pools[1][2], pools[2][2]) and pools[2][0].shape[0] > pools[1][0].shape[0]
    outs = [run(q, kp, vp, bt, lens, ks, vs) for (kp, vp, bt) in pools]
    check(outs[0][0], outs[0][1], q, *pools[0], lens, ks, vs, "identity order D=%d %s" % (D, shape))
    for o, lse in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (2, 1, 8, 128, 8), (3, 5, 1, 32, 2)], ids=ids)
def test_nothing_outside_the_live_rows_is_used(built, dev, shape, D):
    B, Hkv, G, page, mp = shape
    S, C, need = plan_of(shape, D)
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    lens = [C + 1, page * mp - 1, 5][:B] if S > 1 else [page + 1, page * mp - 1, 5][:B]
    assert all(n % page for n in lens)  # every last live page has rows at or past the length
    plain_pool = f8.make_pool(k8, v8, page, lens)
    plain = run(q, *plain_pool, lens, ks, vs)
    for fill in (f8.NAN_BYTE, 0x7E):  # NaN, and the largest finite value: 448 scale
        kf, vf = bits(k8).clone(), bits(v8).clone()
        for b in range(B):
            kf[b, :, lens[b]:] = fill
            vf[b, :, lens[b]:] = fill
        kp, vp, bt = f8.make_pool(kf.view(f8.F8), vf.view(f8.F8), page, lens)
        assert torch.equal(bt, plain_pool[2])
        kd, vd = kp.to(dev), vp.to(dev)
        ws = torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device=dev)
        o, lse = run(q, kd, vd, bt, lens, ks, vs, workspace=ws)
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
        assert torch.equal(o, plain[0]) and torch.equal(lse, plain[1])
        assert torch.equal(bits(kd.cpu()), bits(kp)) and torch.equal(bits(vd.cpu()), bits(vp))  # the caches are inputs: bit-unchanged
    check(plain[0], plain[1], q, *plain_pool, lens, ks, vs, "D=%d %s lens=%s" % (D, shape, lens))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (3, 2, 1, 16, 63), (3, 5, 1, 32, 2)], ids=ids)
def test_guard_bands_and_workspaces(built, dev, shape, D):
    """Nothing is written around o, lse and the workspace; a caller's workspace and the one the Python entry allocates give the same bits."""
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp = shape
    Hq, Nmax = Hkv * G, page * mp
    S, C, need = pkg.fa2_decode_paged_fp8_plan(B, Hq, Hkv, mp, page, D)
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    lens = [Nmax, 1, Nmax // 2][:B]
    kp, vp, bt = f8.make_pool(k8, v8, page, lens)
    GB = 256
    ob = torch.full((B * Hq * D + 2 * GB,), 777.0, dtype=torch.half, device=dev)
    lb = torch.full((B * Hq + 2 * GB,), 777.0, dtype=torch.float32, device=dev)
    wb = torch.full((need + 2 * GB,), 0xA5, dtype=torch.uint8, device=dev)
    o, lse, ws = ob[GB:GB + B * Hq * D].view(B, Hq, D), lb[GB:GB + B * Hq].view(B, Hq), wb[GB:GB + need]
    assert ws.numel() == need
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    pkg.fa2_decode_paged_fp8(q.to(dev), kp.to(dev), vp.to(dev), bt.to(dev), sl, ks.to(dev), vs.to(dev), o, lse, ws if need else None)
    torch.cuda.synchronize()
    for buf, n in ((ob, B * Hq * D), (lb, B * Hq)):
        assert bool((buf[:GB] == 777.0).all()) and bool((buf[GB + n:] == 777.0).all())
    assert bool((wb[:GB] == 0xA5).all()) and bool((wb[GB + need:] == 0xA5).all())
    check(o.cpu(), lse.cpu(), q, kp, vp, bt, lens, ks, vs, "guarded D=%d %s" % (D, shape))
    auto = run(q, kp, vp, bt, lens, ks, vs)  # the workspace allocated by the entry
    assert torch.equal(auto[0], o.cpu()) and torch.equal(auto[1], lse.cpu())


@pytest.mark.parametrize("D", DS)
def test_one_hot_keys_select_one_value_row(built, dev, D):
    N, page, G = 4096, 16, 2  # (1, 1, ...): the plan splits the keys 16 ways
    assert f8.plan(1, G, 1, N // page, page, D)[0] >= 3
    _, k, v, _, _ = onehot_problem(N, D, False, seed=5)
    ks, vs = torch.tensor([0.5]), torch.tensor([0.25])  # keys +-1 are the codes +-2; values: e4m3 codes times 1/4
    k8 = f8.quantize(k.view(1, 1, N, D), f8.per_head(ks))
    v8 = f8.quantize(v.view(1, 1, N, D), f8.per_head(vs))
    assert torch.equal(f8.dequantize(k8, f8.per_head(ks)).half().view(N, D), k)
    vq = f8.dequantize(v8, f8.per_head(vs)).half().view(N, D)  # exact: three mantissa bits times a power of two
    bits_ = (N - 1).bit_length()
    score = 16.0 * (D // bits_) * bits_ / D ** 0.5
    for n, ts in ((N, (0, N - 1)), (3000, (2999, 1234)), (257, (256, 17))):
        kp, vp, bt = f8.make_pool(k8, v8, page, [n], seed=n)
        q = torch.stack([k[t] * 16 for t in ts]).view(1, G, D)  # the two heads of the group select different keys
        o, lse = run(q, kp, vp, bt, [n], ks, vs)
        for h, t in enumerate(ts):
            assert torch.equal(o[0, h], vq[t]), (D, n, t)
            assert abs(lse[0, h].item() - score) <= 1e-5 * score, (D, n, t, lse[0, h].item(), score)


@pytest.mark.parametrize("D", DS)
def test_constant_values_zero_query_and_single_key(built, dev, D):
    shape = (3, 1, 4, 32, 32)
    B, Hkv, G, page, mp = shape
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    lens = [1000, 385, 77]
    p2 = torch.tensor([0.125])
    # constant V: the code of 3 under the scale 1/8 is 0.375 everywhere; every accumulator sums terms c p in fp32, far below half an fp16 ulp of c
    vc = torch.full(v8.shape, 3.0).to(f8.F8)
    kp, vp, bt = f8.make_pool(k8, vc, page, lens)
    o, _ = run(q, kp, vp, bt, lens, ks, p2)
    assert bool((o == 0.375).all())
    # q = 0: the mean of the live dequantised rows, LSE = ln(len)
    kp, vp, bt = f8.make_pool(k8, v8, page, lens)
    o, lse = run(torch.zeros_like(q), kp, vp, bt, lens, ks, vs)
    vd = f8.dequantize(v8, f8.per_head(vs), torch.float64)
    for b in range(B):
        mean = vd[b, :, :lens[b]].mean(dim=1).repeat_interleave(G, dim=0)
        assert (o[b].double() - mean).abs().max().item() <= dr.fa_tol(mean), (D, b)
        ln = torch.log(torch.tensor(float(lens[b]), dtype=torch.float64)).item()
        assert (lse[b].double() - ln).abs().max().item() <= 1e-6 * ln, (D, b, lse[b], ln)
    # one key: O = its V row times v_scale bit for bit (a power of two: exact in fp16) for every head of a group; LSE = q . K_0 k_scale / sqrt(D),
    # an fp32 dot product of D exact products and two more roundings for the scale (error <= (D + 6) 2^-24 sum|q_i k_i| / sqrt(D))
    kp, vp, bt = f8.make_pool(k8, v8, page, [1] * B)
    o, lse = run(q, kp, vp, bt, [1] * B, ks, p2)
    k0 = f8.dequantize(k8[:, :, 0], ks.view(-1, 1), torch.float64).repeat_interleave(G, dim=1)
    v0 = (v8[:, :, 0].float() * 0.125).half().repeat_interleave(G, dim=1)
    assert torch.equal(o, v0)
    s = (q.double() * k0).sum(-1) / D ** 0.5
    bound = (D + 6) * 2.0 ** -24 * (q.double() * k0).abs().sum(-1) / D ** 0.5
    assert bool(((lse.double() - s).abs() <= bound).all()), (D, (lse.double() - s).abs().max().item(), bound.min().item())


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (3, 5, 1, 32, 2)], ids=ids)
def test_scale_algebra_bit_for_bit(built, dev, shape, D):
    B, Hkv, G, page, mp = shape
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    lens = [page * mp - 3, page * mp // 2 + 1, 7][:B]
    kp, vp, bt = f8.make_pool(k8, v8, page, lens)
    kd, vd, bd = kp.to(dev), vp.to(dev), bt.to(dev)
    base = run(q, kd, vd, bd, lens, ks, vs)
    h = Hkv - 1
    grp = slice(h * G, (h + 1) * G)
    # k_scale[h] doubled, the q rows of that head's group halved: the same scores bit for bit (q ~ N(0, 1): halving stays in fp16's normal range
    # but for elements below 2^-13, which are set to zero in both runs)
    qn = q.clone()
    qn[qn.abs() < 2.0 ** -12] = 0
    base_n = run(qn, kd, vd, bd, lens, ks, vs)
    k2, q2 = ks.clone(), qn.clone()
    k2[h] *= 2
    q2[:, grp] = qn[:, grp] / 2
    assert torch.equal(q2[:, grp].float() * 2, qn[:, grp].float())
    o, lse = run(q2, kd, vd, bd, lens, k2, vs)
    assert torch.equal(o, base_n[0]) and torch.equal(lse, base_n[1])
    # v_scale[h] doubled: O of that group doubles exactly (|O| ~ 0.1 .. 1: normal in fp16), everything else and every LSE unchanged
    v2 = vs.clone()
    v2[h] *= 2
    o, lse = run(q, kd, vd, bd, lens, ks, v2)
    want = base[0].clone()
    want[:, grp] = base[0][:, grp] * 2
    tiny = base[0][:, grp].abs() < 2.0 ** -14  # a subnormal fp16 result has lost bits that the doubled one keeps
    assert bool((o[:, grp][~tiny] == want[:, grp][~tiny]).all()) and int(tiny.sum()) <= max(1, tiny.numel() // 100)
    rest = [i for i in range(Hkv * G) if not (h * G <= i < (h + 1) * G)]
    assert torch.equal(o[:, rest], base[0][:, rest]) and torch.equal(lse, base[1])
    if Hkv >= 2:  # swapping two heads' scales changes those heads only
        for which in ("k", "v"):
            sw = (ks if which == "k" else vs).clone()
            sw[0], sw[h] = sw[h].clone(), sw[0].clone()
            o, lse = run(q, kd, vd, bd, lens, sw if which == "k" else ks, sw if which == "v" else vs)
            mid = [i for i in range(Hkv * G) if G <= i < h * G]
            assert torch.equal(o[:, mid], base[0][:, mid]) and torch.equal(lse[:, mid], base[1][:, mid])
            assert not torch.equal(o[:, :G], base[0][:, :G]) and not torch.equal(o[:, grp], base[0][:, grp])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(2, 2, 4, 16, 64), (2, 1, 8, 128, 8), (1, 1, 8, 16, 1)], ids=ids)
def test_heads_of_a_group_are_independent_and_equal_queries_give_equal_bits(built, dev, shape, D):
    B, Hkv, G, page, mp = shape
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    lens = [page * mp - 3, page * mp // 2 + 1][:B]
    kp, vp, bt = f8.make_pool(k8, v8, page, lens)
    kd, vd, bd = kp.to(dev), vp.to(dev), bt.to(dev)
    base = run(q, kd, vd, bd, lens, ks, vs)
    q2 = q.clone()
    q2[:, 1::G] = problem(shape, D, seed=1)[0][:, 1::G]  # head 1 of every group
    other = run(q2, kd, vd, bd, lens, ks, vs)
    keep = [h for h in range(Hkv * G) if h % G != 1]
    assert torch.equal(base[0][:, keep], other[0][:, keep]) and torch.equal(base[1][:, keep], other[1][:, keep])
    assert not torch.equal(base[0][:, 1::G], other[0][:, 1::G])
    qe = q[:, ::G].repeat_interleave(G, dim=1)  # all G queries of a group equal
    o, lse = run(qe, kd, vd, bd, lens, ks, vs)
    o, lse = o.view(B, Hkv, G, D), lse.view(B, Hkv, G)
    assert all(torch.equal(o[:, :, h], o[:, :, 0]) and torch.equal(lse[:, :, h], lse[:, :, 0]) for h in range(G))
    assert torch.equal(o[:, :, 0], base[0][:, ::G])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 2, 1, 16, 63), (2, 1, 8, 128, 8), (3, 5, 1, 32, 2)], ids=ids)
def test_lengths_are_clamped(built, dev, shape, D):
    B, Hkv, G, page, mp = shape
    Nmax = page * mp
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    kp, vp, bt = f8.make_pool(k8, v8, page, [Nmax] * B)
    kd, vd, bd = kp.to(dev), vp.to(dev), bt.to(dev)
    o, lse = run(q, kd, vd, bd, [0, -3, 0][:B], ks, vs)
    assert bool((o == 0).all()) and bool((lse == float("-inf")).all())
    full = run(q, kd, vd, bd, [Nmax] * B, ks, vs)
    over = run(q, kd, vd, bd, [Nmax + 7] * B, ks, vs)
    assert torch.equal(full[0], over[0]) and torch.equal(full[1], over[1])
    mixed = run(q, kd, vd, bd, [0, Nmax + 7, -3][:B], ks, vs)
    assert bool((mixed[0][0] == 0).all()) and torch.equal(mixed[0][1], full[0][1]) and torch.equal(mixed[1][1], full[1][1])
    assert mixed[1][0].tolist() == [float("-inf")] * (Hkv * G)
    check(full[0], full[1], q, kp, vp, bt, [Nmax] * B, ks, vs, "full D=%d %s" % (D, shape))


@pytest.mark.parametrize("D", DS)
def test_a_sequence_does_not_depend_on_its_neighbours_and_calls_repeat(built, dev, D):
    import cuda_learn_notes_amd as pkg
    shape = (3, 1, 4, 32, 32)
    B, Hkv, G, page, mp = shape
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    lens = [700, 999, 333]
    kp, vp, bt = f8.make_pool(k8, v8, page, lens, seed=3)
    first = run(q, kp, vp, bt, lens, ks, vs)
    # other lengths, other data and other pages for sequences 0 and 2; sequence 1 keeps its logical rows but moves in the pool
    k2, v2 = (bits(t).clone() for t in problem(shape, D, seed=1)[1:3])
    k2[1], v2[1] = bits(k8)[1], bits(v8)[1]
    lens2 = [1, 999, 1024]
    kp2, vp2, bt2 = f8.make_pool(k2.view(f8.F8), v2.view(f8.F8), page, lens2, seed=4)
    other = run(q, kp2, vp2, bt2, lens2, ks, vs)
    assert not torch.equal(bt[1], bt2[1])
    assert torch.equal(first[0][1], other[0][1]) and torch.equal(first[1][1], other[1][1])
    assert not torch.equal(first[0][0], other[0][0])
    qd, kd, vd, bd, ksd, vsd = (t.to(dev) for t in (q, kp, vp, bt, ks, vs))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    ws = torch.empty(max(pkg.fa2_decode_paged_fp8_plan(B, Hkv * G, Hkv, mp, page, D)[2], 16), dtype=torch.uint8, device=dev)
    outs = [(torch.empty_like(qd), torch.empty(B, Hkv * G, dtype=torch.float32, device=dev)) for _ in range(20)]
    for o, l in outs:
        pkg.fa2_decode_paged_fp8(qd, kd, vd, bd, sl, ksd, vsd, o, l, ws)
    torch.cuda.synchronize()
    assert all(torch.equal(o.cpu(), first[0]) and torch.equal(l.cpu(), first[1]) for o, l in outs)


def check_appended(gk, gv, qo, before_k, ref, bt, lens, T, page, ks, what):
    """What an append left on the GPU against the reference chain: V bytes equal; every K byte outside the step's live rows as before the step;
    every element of the live K rows within fp8_kv_reference.bound of the fp64 rotation (+-448 exactly beyond the clamp); q_out within
    kv_append_reference.bound."""
    assert torch.equal(bits(gv), bits(ref.v_pages)), what
    keep = ~ref.k_live[:, None, :, None].expand_as(gk)
    assert torch.equal(bits(gk)[keep], bits(before_k)[keep]), what
    s64 = ks.double().view(-1, 1)
    worst = 0.0
    assert ref.live, what
    for (b, t) in ref.live:
        pos = int(lens[b]) - T + t
        got = f8.dequantize(gk[int(bt[b, pos // page]), :, pos % page], s64, torch.float64)
        y, mag = ref.k_rot[b, t], ref.k_mag[b, t]
        inside = y.abs() <= 448.0 * s64
        worst = max(worst, ((got - y).abs() / f8.bound(y, s64, mag))[inside].max().item())
        assert bool((got[~inside] == (448.0 * s64 * y.sign())[~inside]).all()), (what, b, t)
    qworst = ((qo.double() - ref.q_rot).abs() / kr.bound(ref.q_rot, ref.q_mag)).max().item()
    differ = int((bits(gk) != bits(ref.k_pages)).sum())
    print("%s: K worst error / bound %.4f, q_out %.4f; %d K bytes differ from quantize(fp64 rotation)" % (what, worst, qworst, differ))
    assert worst <= 1.0 and qworst <= 1.0, (what, worst, qworst)


def chain_problem(D, steps, seed):
    """One stream of decode steps with Hkv = 2, G = 4, page 16: fp16 k_new, v_new [steps][B,1,Hkv,D] and q [steps][B,1,Hq,D], the start lengths,
    the scales, a block table over distinct pages, and the rope table."""
    import cuda_learn_notes_amd as pkg
    B, Hkv, Hq, page, mp = 3, 2, 8, 16, 4
    g = torch.Generator().manual_seed(seed + D)
    kn, vn = (torch.randn(steps, B, 1, Hkv, D, generator=g).half() for _ in range(2))
    q = torch.randn(steps, B, 1, Hq, D, generator=g).half()
    P = B * mp + 3
    bt = torch.randperm(P, generator=g)[:B * mp].view(B, mp).to(torch.int32)
    return kn, vn, q, [0, 14, 40], scales_for(Hkv, "k") * 1.3, scales_for(Hkv, "v") * 1.3, bt, pkg.kv_append_rope_table(mp * page, D), P


@pytest.mark.parametrize("D", DS)
def test_append_then_decode_over_several_steps_against_the_reference_chain(built, dev, D):
    """kv_append_paged_fp8 (rope "half") then fa2_decode_paged_fp8 on one stream, step after step, against the reference chain: ref_append_fp8
    from the pools of the previous reference step, never from what the GPU wrote. After every step the GPU's V bytes equal the chain's, its
    live K rows lie within fp8_kv_reference.bound of the chain's fp64 rotation (a byte may sit one code off where the fp32 rotation crosses
    a rounding boundary), every other K byte is what the GPU held before the step, and q_out is within kv_append_reference.bound. The
    attention of the step is then held to the reference on those checked pools."""
    import cuda_learn_notes_amd as pkg
    steps = 6
    kn, vn, q, len0, ks, vs, bt, table, P = chain_problem(D, steps, seed=11)
    B, _, Hkv, _ = kn.shape[1:]
    page = 16
    g = torch.Generator().manual_seed(D)  # the history in front of the start lengths: any codes but the NaN ones
    kp, vp = ((torch.randint(0, 0x7F, (P, Hkv, page, D), generator=g) | (torch.randint(0, 2, (P, Hkv, page, D), generator=g) << 7))
              .to(torch.uint8).view(f8.F8) for _ in range(2))
    kd, vd, bd, ksd, vsd, td = (t.to(dev) for t in (kp, vp, bt, ks, vs, table))
    rk, rv, gk_before = kp, vp, kp
    for s in range(steps):
        lens = [n + s + 1 for n in len0]  # the lengths count the new token
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        qo = torch.full(q[s].shape, float("nan"), dtype=torch.half, device=dev)
        pkg.kv_append_paged_fp8(kn[s].to(dev), vn[s].to(dev), kd, vd, bd, sl, ksd, vsd, q[s].to(dev), qo, td, "half")
        o = torch.full((B, q.shape[3], D), float("nan"), dtype=torch.half, device=dev)
        lse = torch.full((B, q.shape[3]), float("nan"), dtype=torch.float32, device=dev)
        pkg.fa2_decode_paged_fp8(qo.view(B, -1, D), kd, vd, bd, sl, ksd, vsd, o, lse)
        torch.cuda.synchronize()
        ref = f8.ref_append_fp8(kn[s], vn[s], rk, rv, bt, lens, ks, vs, q[s], table, 1)
        assert len(ref.live) == B
        check_appended(kd.cpu(), vd.cpu(), qo.cpu(), gk_before, ref, bt, lens, 1, page, ks, "chain D=%d step %d" % (D, s))
        rk, rv, gk_before = ref.k_pages, ref.v_pages, kd.cpu()
        check(o.cpu(), lse.cpu(), qo.cpu().view(B, -1, D), kd.cpu(), vd.cpu(), bt, lens, ks, vs, "chain D=%d step %d" % (D, s))
    assert not torch.equal(bits(rk), bits(kp))


@pytest.mark.parametrize("D", DS)
def test_graph_replay_of_the_step_reads_everything_from_the_device(built, dev, D):
    """Append and attention (and the merge of its splits) captured once as one line of kernels on one stream; lengths, table, scales, pools, new
    rows and q changed in place; the replay equals the eager step on the same device state bit for bit, and the reference."""
    import cuda_learn_notes_amd as pkg
    B, Hkv, Hq, page, mp = 2, 2, 8, 16, 64
    S, C, need = pkg.fa2_decode_paged_fp8_plan(B, Hq, Hkv, mp, page, D)
    assert S > 1  # three kernels in a line
    shape = (B, Hkv, Hq // Hkv, page, mp)
    _, k8, v8, ks, vs, _, _ = problem(shape, D)
    Nmax = page * mp
    g = torch.Generator().manual_seed(17 + D)
    table = pkg.kv_append_rope_table(Nmax, D)
    state = []
    for i, lens in enumerate(([100, Nmax], [900, 513])):
        kp, vp, bt = f8.make_pool(k8, v8, page, [Nmax] * B, seed=i + 1)  # both pools hold every page of both sequences
        kn, vn = (torch.randn(B, 1, Hkv, D, generator=g).half() for _ in range(2))
        q = torch.randn(B, 1, Hq, D, generator=g).half()
        state.append((kp, vp, bt, kn, vn, q, lens, ks * (1 + i), vs * (1 + 0.5 * i)))
    assert state[0][0].shape == state[1][0].shape and not torch.equal(state[0][2], state[1][2])
    kp, vp, bt, kn, vn, q, lens, s_k, s_v = state[0]
    kd, vd, bd, knd, vnd, qd, ksd, vsd, td = (t.to(dev).clone() for t in (kp, vp, bt, kn, vn, q, s_k, s_v, table))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    qo, og = torch.zeros_like(qd), torch.zeros(B, Hq, D, dtype=torch.half, device=dev)
    lg = torch.zeros(B, Hq, dtype=torch.float32, device=dev)

    def step(kpool, vpool, q_out, o, lse):
        pkg.kv_append_paged_fp8(knd, vnd, kpool, vpool, bd, sl, ksd, vsd, qd, q_out, td, "half")
        pkg.fa2_decode_paged_fp8(q_out.view(B, Hq, D), kpool, vpool, bd, sl, ksd, vsd, o, lse, ws)

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        step(kd, vd, qo, og, lg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(kd, vd, qo, og, lg)
    kp, vp, bt, kn, vn, q, lens, s_k, s_v = state[1]
    sl.copy_(torch.tensor(lens, dtype=torch.int32))
    kd.copy_(kp), vd.copy_(vp), bd.copy_(bt), knd.copy_(kn), vnd.copy_(vn), qd.copy_(q), ksd.copy_(s_k), vsd.copy_(s_v)
    qo.zero_(), og.zero_(), lg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    ke, ve = kp.to(dev), vp.to(dev)
    qe, oe, le = torch.empty_like(qd), torch.empty_like(og), torch.empty_like(lg)
    step(ke, ve, qe, oe, le)
    torch.cuda.synchronize()
    assert torch.equal(bits(kd), bits(ke)) and torch.equal(bits(vd), bits(ve)) and torch.equal(qo, qe) and torch.equal(og, oe) and torch.equal(lg, le)
    assert not torch.equal(bits(kd.cpu()), bits(kp))  # the replay appended
    ref = f8.ref_append_fp8(kn, vn, kp, vp, bt, lens, s_k, s_v, q, table, 1)
    check_appended(kd.cpu(), vd.cpu(), qo.cpu(), kp, ref, bt, lens, 1, page, s_k, "graph replay D=%d" % D)
    check(og.cpu(), lg.cpu(), qo.cpu().view(B, Hq, D), kd.cpu(), vd.cpu(), bt, lens, s_k, s_v, "graph replay D=%d" % D)


def test_python_argument_errors(built, dev):
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp, D = 2, 2, 4, 16, 64, 64
    Hq, P = Hkv * G, 200
    q = torch.zeros(B, Hq, D, dtype=torch.half, device=dev)
    kp = torch.zeros(P, Hkv, page, D, dtype=torch.uint8, device=dev).view(f8.F8)
    vp = kp.clone()
    bt = torch.zeros(B, mp, dtype=torch.int32, device=dev)
    sl = torch.tensor([5, 9], dtype=torch.int32, device=dev)
    ks, vs = torch.ones(Hkv, device=dev), torch.ones(Hkv, device=dev)
    o = torch.empty_like(q)
    f = pkg.fa2_decode_paged_fp8
    need = pkg.fa2_decode_paged_fp8_plan(B, Hq, Hkv, mp, page, D)[2]
    assert need > 0
    f(q, kp, vp, bt, sl, ks, vs, o)
    bad = [
        lambda: f(q, kp.view(torch.uint8).half(), vp.view(torch.uint8).half(), bt, sl, ks, vs, o),   # fp16 pools: the other entry's
        lambda: f(q, kp.view(torch.uint8), vp, bt, sl, ks, vs, o),                                  # bytes that are no e4m3 tensor
        lambda: f(q, kp, vp.view(torch.float8_e5m2), bt, sl, ks, vs, o),
        lambda: f(q.float(), kp, vp, bt, sl, ks, vs, o),
        lambda: f(q, kp, vp, bt, sl, ks.cpu(), vs, o),                                              # scales on the CPU
        lambda: f(q, kp, vp, bt, sl, ks, vs.cpu(), o),
        lambda: f(q, kp, vp, bt, sl, ks[:1], vs, o),                                                # scale shape
        lambda: f(q, kp, vp, bt, sl, ks, torch.ones(Hkv, 1, device=dev), o),
        lambda: f(q, kp, vp, bt, sl, ks, torch.ones(Hq, device=dev), o),
        lambda: f(q, kp, vp, bt, sl, ks.half(), vs, o),                                             # scale dtype
        lambda: f(q, kp, vp, bt, sl, ks, vs.double(), o),
        lambda: f(q, kp, vp, bt.long(), sl, ks, vs, o),
        lambda: f(q, kp, vp, bt, sl.cpu(), ks, vs, o),
        lambda: f(q, kp, vp[:100].contiguous(), bt, sl, ks, vs, o),
        lambda: f(q, kp, vp, bt, sl, ks, vs, o, lse=torch.empty(B, Hq + 1, dtype=torch.float32, device=dev)),
        lambda: f(q, kp, vp, bt, sl, ks, vs, o, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev)),  # short workspace
    ]
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
    q6 = torch.zeros(B, 6, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match="group size 3"):
        f(q6, kp, vp, bt, sl, ks, vs, torch.empty_like(q6))
    kp48 = torch.zeros(P, Hkv, 48, D, dtype=torch.uint8, device=dev).view(f8.F8)
    with pytest.raises(RuntimeError, match="page size 48"):
        f(q, kp48, kp48.clone(), bt, sl, ks, vs, o)
