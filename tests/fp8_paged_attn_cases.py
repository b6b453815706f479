"""The GPU cases that tests/test_gpu_fa2_prefill_paged_fp8.py and tests/test_gpu_fa2_decode_paged_multi_fp8.py share: both entries take the same
tensors ([B,T,Hq,D] queries over e4m3fn pools with per-head scales) and promise the same things, so a case is written once against an Entry
(which entry to call, its fp64 reference on the DEQUANTISED pools, its shapes) and each test file runs it for its entry. The bounds are
decode_reference.fa_tol / lse_tol unchanged: the codes are exact in fp16 and the scales enter in fp32, so the kernels' error against that
reference is that of the fp16 kernels. Pools come from fp8_kv_reference.make_pool (unused pages and the poison page hold the NaN byte 0x7f).
Every case prints its figures before it asserts (pytest -s). A plain module: nothing here is collected."""
import functools

import torch

import decode_reference as dr
import fp8_kv_reference as f8
import fp8_paged_attn_reference as fr
import kv_append_reference as kr
from fa_reference import onehot_problem

bits = f8.bits
FINITE_CODES = [c for c in range(256) if c & 0x7F != 0x7F]  # the 254 bytes that are no NaN code


def scales_for(Hkv, which):
    """Per-head scales that differ across heads, near absmax / 448 of N(0, 1) data (those of tests/test_gpu_fa2_decode_paged_fp8.py)."""
    base = 0.0101 if which == "k" else 0.0093
    return torch.tensor([base * (1.0 + 0.37 * h) for h in range(Hkv)])


class Entry:
    """kind "prefill": fa2_prefill_paged_fp8 (no workspace); kind "multi": fa2_decode_paged_multi_fp8 (T <= 8, a split plan)."""

    def __init__(self, kind):
        self.kind, self.multi = kind, kind == "multi"
        self.name = "fa2_decode_paged_multi_fp8" if self.multi else "fa2_prefill_paged_fp8"
        self.fp16_name = "fa2_decode_paged_multi" if self.multi else "fa2_prefill_paged"
        self.ref = fr.ref_decode_paged_multi_fp8 if self.multi else fr.ref_prefill_paged_fp8

    def need(self, shape, D):
        B, Hkv, G, page, mp, T = shape
        return fr.plan(B, T, Hkv * G, Hkv, mp, page, D)[2] if self.multi else 0

    def call(self, q, kp, vp, bt, sl, ks, vs, o, lse=None, ws=None):
        import cuda_learn_notes_amd as pkg
        if self.multi:
            pkg.fa2_decode_paged_multi_fp8(q, kp, vp, bt, sl, ks, vs, o, lse, ws)
        else:
            pkg.fa2_prefill_paged_fp8(q, kp, vp, bt, sl, ks, vs, o, lse)

    def call_fp16(self, q, kp, vp, bt, sl, o, lse=None):
        import cuda_learn_notes_amd as pkg
        getattr(pkg, self.fp16_name)(q, kp, vp, bt, sl, o, lse)

    def run(self, q, kp, vp, bt, lens, ks, vs, want_lse=True, workspace=None, dev="cuda"):
        qd, kd, vd, bd, ksd, vsd = (t.to(dev) if not t.is_cuda else t for t in (q, kp, vp, bt, ks, vs))
        sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
        o = torch.full_like(qd, float("nan"))
        lse = torch.full(qd.shape[:3], float("nan"), dtype=torch.float32, device=dev) if want_lse else None
        self.call(qd, kd, vd, bd, sl, ksd, vsd, o, lse, workspace)
        torch.cuda.synchronize()
        return o.cpu(), (lse.cpu() if want_lse else None)

    def check(self, o, lse, q, kp, vp, bt, lens, ks, vs, what, ref=None):
        """O within fa_tol(ref), LSE within lse_tol(ref) of the reference on the dequantised pools, -inf LSE entries and their zero rows exactly;
        returns the two ratios error / bound."""
        ro, rl = ref if ref is not None else self.ref(q, kp, vp, ks, vs, bt, lens)
        assert bool(torch.isfinite(o).all()), what
        eo, bo = (o.double() - ro).abs().max().item(), dr.fa_tol(ro)
        fin = torch.isfinite(rl)
        assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float("-inf")).all()), what
        assert bool((o[~fin] == 0).all()), what  # a query that sees no key
        el = (lse.double()[fin] - rl[fin]).abs().max().item() if bool(fin.any()) else 0.0
        bl = dr.lse_tol(rl)
        print("%s %s: O err %.3e / bound %.3e = %.4f   LSE err %.3e / bound %.3e = %.4f" % (self.kind, what, eo, bo, eo / bo, el, bl, el / bl))
        assert eo <= bo, (what, eo, bo)
        assert el <= bl, (what, el, bl)
        return eo / bo, el / bl


@functools.lru_cache(maxsize=None)
def problem(shape, D, seed=0):
    """On the CPU, made once per shape and never modified: q fp16 [B,T,Hq,D]; Gaussian dense k, v fp32 [B,Hkv,Nmax,D] and their e4m3 forms k8, v8
    under the per-head scales ks, vs. Returns (q, k8, v8, ks, vs, k, v)."""
    B, Hkv, G, page, mp, T = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * Hkv + 17 * G + page * mp + D + 31 * T)
    q = torch.randn(B, T, Hkv * G, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, page * mp, D, generator=g) for _ in range(2))
    ks, vs = scales_for(Hkv, "k"), scales_for(Hkv, "v")
    return q, f8.quantize(k, f8.per_head(ks)), f8.quantize(v, f8.per_head(vs)), ks, vs, k, v


def pool_run_check(e, shape, D, lens, what, seed=0):
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    kp, vp, bt = f8.make_pool(k8, v8, shape[3], lens, seed=seed)
    o, lse = e.run(q, kp, vp, bt, lens, ks, vs)
    return (o, lse) + e.check(o, lse, q, kp, vp, bt, lens, ks, vs, what)


# ---- 1: parity


def parity(e, shape, D, lengths):
    B, Hkv, G, page, mp, T = shape
    worst = (0.0, 0.0)
    for i, n in enumerate(lengths):
        r = pool_run_check(e, shape, D, [n] * B, "D=%d %s len=%d" % (D, shape, n), seed=i)[2:]
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("%s D=%d %s: worst error / bound  O %.4f  LSE %.4f" % ((e.kind, D, shape) + worst))
    # what the cache format costs on this data, against the un-quantised fp64 answer: printed, not asserted
    q, k8, v8, ks, vs, k, v = problem(shape, D)
    lens = [page * mp] * B
    ident = torch.arange(B * mp, dtype=torch.int32).view(B, mp)
    as_pool = lambda t: t.view(B, Hkv, mp, page, D).permute(0, 2, 1, 3, 4).reshape(B * mp, Hkv, page, D)  # noqa: E731
    one = torch.ones(Hkv)
    ro, _ = e.ref(q, as_pool(k), as_pool(v), one, one, ident, lens)
    rq, _ = e.ref(q, as_pool(bits(k8)).view(f8.F8), as_pool(bits(v8)).view(f8.F8), ks, vs, ident, lens)
    print("%s D=%d %s: quantisation error of O at len %d: max %.3e (max|O| %.3e)"
          % (e.kind, D, shape, lens[0], (rq - ro).abs().max().item(), ro.abs().max().item()))


def mixed_empty_and_clamped(e, shape, D, mid):
    """The ragged batch (length 1 < T right-aligned, `mid`, capacity), the empty sequence, and lengths clamped at 0 and at the capacity."""
    B, Hkv, G, page, mp, T = shape
    Nmax = page * mp
    assert B >= 3 and T >= 2
    lens = [1, mid, Nmax]
    o, lse, _, _ = pool_run_check(e, shape, D, lens, "D=%d %s lens=%s" % (D, shape, lens))
    assert bool((lse[0, :T - 1] == float("-inf")).all()) and bool(torch.isfinite(lse[0, T - 1]).all()) and bool(torch.isfinite(lse[2]).all())
    assert bool((o[0, :T - 1] == 0).all())
    lens = [Nmax - 7, 0, T + 40]
    o, lse, _, _ = pool_run_check(e, shape, D, lens, "D=%d %s lens=%s" % (D, shape, lens))
    assert bool((o[1] == 0).all()) and bool((lse[1] == float("-inf")).all()) and bool(torch.isfinite(lse[0]).all())
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    kp, vp, bt = f8.make_pool(k8, v8, page, [Nmax] * B)
    kd, vd, bd = kp.cuda(), vp.cuda(), bt.cuda()
    o, lse = e.run(q, kd, vd, bd, [0, -3, 0], ks, vs)
    assert bool((o == 0).all()) and bool((lse == float("-inf")).all())
    full = e.run(q, kd, vd, bd, [Nmax] * B, ks, vs)
    over = e.run(q, kd, vd, bd, [Nmax + 7] * B, ks, vs)
    assert torch.equal(full[0], over[0]) and torch.equal(full[1], over[1])
    mix = e.run(q, kd, vd, bd, [0, Nmax + 7, -3], ks, vs)
    assert bool((mix[0][0] == 0).all()) and torch.equal(mix[0][1], full[0][1]) and torch.equal(mix[1][1], full[1][1])
    e.check(full[0], full[1], q, kp, vp, bt, [Nmax] * B, ks, vs, "full D=%d %s" % (D, shape))


# ---- 2: every code converts exactly


def all_codes_problem(D, T, G):
    """One-hot keys (fa_reference.onehot_problem: keys +-1, stored as the codes +-2 under k_scale = 0.5), V rows that cycle through the 254
    finite e4m3 bytes, v_scale = 1/4, N = 4096 keys in pages of 16 (the multi plan splits them). For each of three lengths n the queries
    q [1,T,G,D]: query (t, g) selects one key target[t, g] below its own causal edge n - (T - 1 - t) (g = 0: the key AT the edge), so
    O[t, g] = e4m3(V bytes of that key) / 4 and LSE = score. The queries are 32 x the key (onehot_problem uses 16): every other key scores at
    least 2 x 32 r / sqrt(D) >= 40 nats less, so whatever the kernel's merge order lets through of the other rows is at most
    4096 e^-40 x 112 = 2e-12 -- far below 2^-22, half an fp16 ulp of the smallest non-zero expected value 2^-11 (the multi-token kernel merges
    fp32 partials of splits that do not hold the target, so a margin of 20 nats is not enough next to values that span 2^-11 .. 112). The
    selected rows of the three lengths together hold every finite byte (asserted here). Returns (k8, v8, ks, vs, want_v fp16 [N,D], score, [(n, target, q)])."""
    N = 4096
    _, k, _, _, _ = onehot_problem(N, D, False, seed=5)
    ks, vs = torch.tensor([0.5]), torch.tensor([0.25])
    k8 = f8.quantize(k.view(1, 1, N, D), f8.per_head(ks))
    assert torch.equal(f8.dequantize(k8, f8.per_head(ks)).half().view(N, D), k)
    codes = torch.tensor(FINITE_CODES, dtype=torch.uint8)
    idx = torch.arange(N * D)
    v8 = codes[(idx * 37 + idx // D) % 254].view(1, 1, N, D).view(f8.F8)
    want_v = (v8.float() * 0.25).half().view(N, D)  # exact: at most four significant bits times a power of two, >= 2^-11
    assert torch.equal(want_v.double(), v8.float().double().view(N, D) * 0.25)
    nbits = (N - 1).bit_length()
    score = 32.0 * (D // nbits) * nbits / D ** 0.5
    assert 2 * 32.0 * (D // nbits) / D ** 0.5 >= 40.0
    cases, seen = [], set()
    for n in (N, 3000, 257):
        target = torch.zeros(T, G, dtype=torch.int64)
        for t in range(T):
            edge = n - (T - 1 - t)  # the keys query t sees
            for g in range(G):
                target[t, g] = edge - 1 if g == 0 else (7919 * (t * G + g) + 13) % edge
        assert bool((target < (n - (T - 1 - torch.arange(T)))[:, None]).all()) and bool((target >= 0).all())
        seen |= set(bits(v8).view(N, D)[target.flatten()].flatten().tolist())
        cases.append((n, target, (k[target.flatten()] * 32).view(1, T, G, D)))
    assert seen == set(FINITE_CODES), sorted(set(FINITE_CODES) - seen)
    return k8, v8, ks, vs, want_v, score, cases


def every_code_converts_exactly(e, D, T, G):
    """all_codes_problem through the entry: O equals e4m3(code) v_scale bit for bit (every such value is an fp16 value, subnormal codes
    included) and LSE the known score within 1e-5 relative. The sign of a ZERO is not kept by a sum (0 + -0 = +0): where the expected value
    is +-0 the output must be a zero, everywhere else its bits must match."""
    N, page = 4096, 16
    if e.multi:
        assert fr.plan(1, T, G, 1, N // page, page, D)[0] >= 3
    k8, v8, ks, vs, want_v, score, cases = all_codes_problem(D, T, G)
    for n, target, q in cases:
        kp, vp, bt = f8.make_pool(k8, v8, page, [n], seed=n)
        o, lse = e.run(q, kp, vp, bt, [n], ks, vs)
        want = want_v[target.flatten()].view(1, T, G, D)
        zero = want == 0
        wrong = int((o.view(torch.int16)[~zero] != want.view(torch.int16)[~zero]).sum()) + int((o[zero] != 0).sum())
        lerr = ((lse - score).abs() / score).max().item()
        print("%s D=%d len %d: %d of %d elements differ from e4m3(code) v_scale; LSE rel err %.2e" % (e.kind, D, n, wrong, o.numel(), lerr))
        assert wrong == 0, (D, n, wrong)
        assert lerr <= 1e-5, (D, n, lerr)


# ---- 3: the causal tail


def causal_tail_is_masked(e, shape, D, lens, tokens):
    """For each token t of `tokens`: the K and V rows [n(b,t), len_b), which later queries see and query t must not, overwritten with the
    largest-magnitude codes 0x7e (+448) / 0xfe (-448) -- the rows <= t of O and LSE keep their bits."""
    B, Hkv, G, page, mp, T = shape
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    assert all(n >= T for n in lens)
    pool = f8.make_pool(k8, v8, page, lens)
    clean = e.run(q, *pool, lens, ks, vs)
    e.check(clean[0], clean[1], q, *pool, lens, ks, vs, "clean D=%d %s lens=%s" % (D, shape, lens))
    for t in tokens:
        kf, vf = bits(k8).clone(), bits(v8).clone()
        for b in range(B):
            n_bt = lens[b] - (T - 1 - t)
            kf[b, :, n_bt:lens[b]] = 0x7E
            vf[b, :, n_bt:lens[b], 0::2] = 0xFE
            vf[b, :, n_bt:lens[b], 1::2] = 0x7E
        kp, vp, bt = f8.make_pool(kf.view(f8.F8), vf.view(f8.F8), page, lens)
        assert torch.equal(bt, pool[2])
        o, lse = e.run(q, kp, vp, bt, lens, ks, vs)
        assert torch.equal(o[:, :t + 1], clean[0][:, :t + 1]) and torch.equal(lse[:, :t + 1], clean[1][:, :t + 1]), (D, shape, t)
        assert not torch.equal(o[:, t + 1:], clean[0][:, t + 1:])  # the rows behind it do see the change


# ---- 4: nothing outside the live rows


def nothing_outside_the_live_rows(e, shape, D, lens):
    B, Hkv, G, page, mp, T = shape
    need = e.need(shape, D)
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    assert all(n % page for n in lens)  # every last live page has rows at or past the length
    plain_pool = f8.make_pool(k8, v8, page, lens)
    plain = e.run(q, *plain_pool, lens, ks, vs)
    for fill in (f8.NAN_BYTE, 0x7E):  # NaN, and the largest finite value
        kf, vf = bits(k8).clone(), bits(v8).clone()
        for b in range(B):
            kf[b, :, lens[b]:] = fill
            vf[b, :, lens[b]:] = fill
        kp, vp, bt = f8.make_pool(kf.view(f8.F8), vf.view(f8.F8), page, lens)
        assert torch.equal(bt, plain_pool[2])
        kd, vd = kp.cuda(), vp.cuda()
        ws = torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device="cuda") if e.multi else None
        o, lse = e.run(q, kd, vd, bt, lens, ks, vs, workspace=ws)
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse[lse != float("-inf")]).all()) and not bool(torch.isnan(lse).any())
        assert torch.equal(o, plain[0]) and torch.equal(lse, plain[1])
        assert torch.equal(bits(kd.cpu()), bits(kp)) and torch.equal(bits(vd.cpu()), bits(vp))  # the pools are inputs: bit-unchanged
    e.check(plain[0], plain[1], q, *plain_pool, lens, ks, vs, "D=%d %s lens=%s" % (D, shape, lens))


# ---- 5: bit invariance


def placement_neighbours_and_repeats(e, shape, D, lens):
    B, Hkv, G, page, mp, T = shape
    assert B >= 3
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    # identity, two shuffles of the same pool size, and a shuffle in a larger pool
    pools = [f8.make_pool(k8, v8, page, lens, **kw) for kw in (dict(order="identity"), dict(seed=1), dict(seed=3), dict(seed=2, extra=9))]
    tables = [p[2] for p in pools]
    assert all(not torch.equal(tables[i], tables[j]) for i in range(4) for j in range(i))
    assert pools[1][0].shape == pools[2][0].shape and pools[3][0].shape[0] > pools[1][0].shape[0]
    outs = [e.run(q, kp, vp, bt, lens, ks, vs) for (kp, vp, bt) in pools]
    e.check(outs[0][0], outs[0][1], q, *pools[0], lens, ks, vs, "identity order D=%d %s" % (D, shape))
    for o, lse in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1])
    first = outs[0]
    # other queries, other data, other lengths and other pages for sequences 0 and 2; sequence 1 keeps its logical rows but moves in the pool
    q2, k2, v2 = problem(shape, D, seed=1)[:3]
    q2, k2, v2 = q2.clone(), bits(k2).clone(), bits(v2).clone()
    q2[1], k2[1], v2[1] = q[1], bits(k8)[1], bits(v8)[1]
    lens2 = [1, lens[1], page * mp]
    kp2, vp2, bt2 = f8.make_pool(k2.view(f8.F8), v2.view(f8.F8), page, lens2, seed=4)
    other = e.run(q2, kp2, vp2, bt2, lens2, ks, vs)
    assert torch.equal(first[0][1], other[0][1]) and torch.equal(first[1][1], other[1][1])
    assert not torch.equal(first[0][0], other[0][0])
    kp, vp, bt = pools[1]
    qd, kd, vd, bd, ksd, vsd = (t.cuda() for t in (q, kp, vp, bt, ks, vs))
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(e.need(shape, D), 16), dtype=torch.uint8, device="cuda") if e.multi else None
    reps = [(torch.empty_like(qd), torch.empty(B, T, Hkv * G, dtype=torch.float32, device="cuda")) for _ in range(20)]
    for o, l in reps:
        e.call(qd, kd, vd, bd, sl, ksd, vsd, o, l, ws)
    torch.cuda.synchronize()
    assert all(torch.equal(o.cpu(), first[0]) and torch.equal(l.cpu(), first[1]) for o, l in reps)


# ---- 6: scale algebra


def scale_algebra(e, shape, D, lens):
    B, Hkv, G, page, mp, T = shape
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    kp, vp, bt = f8.make_pool(k8, v8, page, lens)
    kd, vd, bd = kp.cuda(), vp.cuda(), bt.cuda()
    base = e.run(q, kd, vd, bd, lens, ks, vs)
    h = Hkv - 1
    grp = slice(h * G, (h + 1) * G)
    # k_scale[h] doubled, the q rows of that head's group halved: the same scores bit for bit (halving stays in fp16's normal range but for
    # elements below 2^-13, which are set to zero in both runs)
    qn = q.clone()
    qn[qn.abs() < 2.0 ** -12] = 0
    base_n = e.run(qn, kd, vd, bd, lens, ks, vs)
    k2, q2 = ks.clone(), qn.clone()
    k2[h] *= 2
    q2[:, :, grp] = qn[:, :, grp] / 2
    assert torch.equal(q2[:, :, grp].float() * 2, qn[:, :, grp].float())
    o, lse = e.run(q2, kd, vd, bd, lens, k2, vs)
    assert torch.equal(o, base_n[0]) and torch.equal(lse, base_n[1])
    # v_scale[h] doubled: O of that group doubles exactly except for subnormal fp16 results, which have lost bits the doubled one keeps. The
    # cap of 1 % on those is checked on the reference first: it is a property of the data, not of the kernel.
    ro, _ = e.ref(q, kp, vp, ks, vs, bt, lens)
    live = ro[:, :, grp].abs().sum(-1, keepdim=True) > 0
    ref_tiny = (ro[:, :, grp].abs() < 2.0 ** -14) & live
    assert int(ref_tiny.sum()) <= ref_tiny.numel() // 200, "the data puts more than 0.5 % of the reference in fp16's subnormal range"
    v2 = vs.clone()
    v2[h] *= 2
    o, lse = e.run(q, kd, vd, bd, lens, ks, v2)
    want = base[0].clone()
    want[:, :, grp] = base[0][:, :, grp] * 2
    tiny = (base[0][:, :, grp].abs() < 2.0 ** -14) & (base[0][:, :, grp] != 0)
    print("%s D=%d %s: %d of %d elements of the group are subnormal in fp16" % (e.kind, D, shape, int(tiny.sum()), tiny.numel()))
    assert bool((o[:, :, grp][~tiny] == want[:, :, grp][~tiny]).all()) and int(tiny.sum()) <= max(1, tiny.numel() // 100)
    rest = [i for i in range(Hkv * G) if not (h * G <= i < (h + 1) * G)]
    assert torch.equal(o[:, :, rest], base[0][:, :, rest]) and torch.equal(lse, base[1])
    if Hkv >= 2:  # swapping two heads' scales changes those heads only (Hkv >= 3: the heads between them are compared)
        for which in ("k", "v"):
            sw = (ks if which == "k" else vs).clone()
            sw[0], sw[h] = sw[h].clone(), sw[0].clone()
            o, lse = e.run(q, kd, vd, bd, lens, sw if which == "k" else ks, sw if which == "v" else vs)
            mid = [i for i in range(Hkv * G) if G <= i < h * G]
            assert torch.equal(o[:, :, mid], base[0][:, :, mid]) and torch.equal(lse[:, :, mid], base[1][:, :, mid])
            assert not torch.equal(o[:, :, :G], base[0][:, :, :G]) and not torch.equal(o[:, :, grp], base[0][:, :, grp])


# ---- 7: the fp16 entry on the same codes


def agrees_with_the_fp16_entry(e, shape, D, lens):
    """The codes as fp16 pools through the fp16 entry, and as e4m3 pools through the FP8 entry with both scales 1: both within the bounds of the
    reference; the differing output bits are printed, not asserted (contraction may differ between two instantiations)."""
    B, Hkv, G, page, mp, T = shape
    q, _, _, _, _, k, v = problem(shape, D)
    one = torch.ones(Hkv)
    k8, v8 = f8.quantize(k, f8.per_head(one)), f8.quantize(v, f8.per_head(one))  # the codes ARE the values, rounded to e4m3: |O| stays ~ 1
    kp, vp, bt = f8.make_pool(k8, v8, page, lens)
    live = bits(kp) != f8.NAN_BYTE
    kh, vh = kp.float().half(), vp.float().half()  # exact; the unused pages hold NaN here too
    assert torch.equal(kh.float()[live], kp.float()[live])
    o8, l8 = e.run(q, kp, vp, bt, lens, one, one)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o16 = torch.full(q.shape, float("nan"), dtype=torch.half, device="cuda")
    l16 = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device="cuda")
    e.call_fp16(q.cuda(), kh.cuda(), vh.cuda(), bt.cuda(), sl, o16, l16)
    torch.cuda.synchronize()
    ref = e.ref(q, kp, vp, one, one, bt, lens)
    e.check(o8, l8, q, kp, vp, bt, lens, one, one, "FP8 entry, scales 1, D=%d %s" % (D, shape), ref=ref)
    e.check(o16.cpu(), l16.cpu(), q, kp, vp, bt, lens, one, one, "fp16 entry on the codes, D=%d %s" % (D, shape), ref=ref)
    print("%s D=%d %s: %d of %d O elements and %d of %d LSE elements differ in bits between the two entries"
          % (e.kind, D, shape, int((o8.view(torch.int16) != o16.cpu().view(torch.int16)).sum()), o8.numel(),
             int((l8.view(torch.int32) != l16.cpu().view(torch.int32)).sum()), l8.numel()))


# ---- 8: across entries


def agree_within_bounds(what, a, b, ref):
    ro, rl = ref
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(a[1]), fin) and torch.equal(torch.isfinite(b[1]), fin), what
    err, lerr = (a[0].float() - b[0].float()).abs().max().item(), ((a[1][fin] - b[1][fin]).abs().max().item() if bool(fin.any()) else 0.0)
    print("%s: O %.3e (bound %.3e)  LSE %.3e (bound %.3e)" % (what, err, dr.fa_tol(ro), lerr, dr.lse_tol(rl)))
    assert err <= dr.fa_tol(ro) and lerr <= dr.lse_tol(rl), what


def prefill_agrees_with_multi(shape, D, lens):
    pre, mul = Entry("prefill"), Entry("multi")
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    assert shape[5] <= 8
    kp, vp, bt = f8.make_pool(k8, v8, shape[3], lens)
    a, b = pre.run(q, kp, vp, bt, lens, ks, vs), mul.run(q, kp, vp, bt, lens, ks, vs)
    ref = pre.ref(q, kp, vp, ks, vs, bt, lens)
    agree_within_bounds("D=%d %s: fa2_prefill_paged_fp8 vs fa2_decode_paged_multi_fp8" % (D, shape), a, b, ref)
    pre.check(a[0], a[1], q, kp, vp, bt, lens, ks, vs, "T=%d D=%d %s" % (shape[5], D, shape), ref=ref)
    mul.check(b[0], b[1], q, kp, vp, bt, lens, ks, vs, "T=%d D=%d %s" % (shape[5], D, shape), ref=ref)


def multi_at_one_token_agrees_with_decode(shape, D, lens):
    import cuda_learn_notes_amd as pkg
    mul = Entry("multi")
    B, Hkv, G, page, mp, T = shape
    assert T == 1
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    kp, vp, bt = f8.make_pool(k8, v8, page, lens)
    a = mul.run(q, kp, vp, bt, lens, ks, vs)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o1 = torch.full((B, Hkv * G, D), float("nan"), dtype=torch.half, device="cuda")
    l1 = torch.full((B, Hkv * G), float("nan"), dtype=torch.float32, device="cuda")
    pkg.fa2_decode_paged_fp8(q[:, 0].contiguous().cuda(), kp.cuda(), vp.cuda(), bt.cuda(), sl, ks.cuda(), vs.cuda(), o1, l1)
    torch.cuda.synchronize()
    ref = mul.ref(q, kp, vp, ks, vs, bt, lens)
    agree_within_bounds("D=%d %s: fa2_decode_paged_multi_fp8 at T = 1 vs fa2_decode_paged_fp8" % (D, shape), a,
                        (o1.cpu().unsqueeze(1), l1.cpu().unsqueeze(1)), ref)
    mul.check(a[0], a[1], q, kp, vp, bt, lens, ks, vs, "T=1 D=%d %s" % (D, shape), ref=ref)
    f8o, f8l = f8.ref_decode_paged_fp8(q[:, 0], kp, vp, ks, vs, bt, lens)
    assert (f8o - ref[0][:, 0]).abs().max().item() <= 1e-12  # the common reference: the two fp64 references agree


# ---- 9: guard bands


def guard_bands_and_workspaces(e, shape, D, lens):
    """Nothing is written around o, lse and (multi) the workspace; a caller's workspace and the one the Python entry allocates give the same
    bits."""
    B, Hkv, G, page, mp, T = shape
    Hq = Hkv * G
    need = e.need(shape, D)
    q, k8, v8, ks, vs, _, _ = problem(shape, D)
    kp, vp, bt = f8.make_pool(k8, v8, page, lens)
    GB, dev = 256, "cuda"
    no, nl = B * T * Hq * D, B * T * Hq
    ob = torch.full((no + 2 * GB,), 777.0, dtype=torch.half, device=dev)
    lb = torch.full((nl + 2 * GB,), 777.0, dtype=torch.float32, device=dev)
    wb = torch.full((need + 2 * GB,), 0xA5, dtype=torch.uint8, device=dev)
    o, lse, ws = ob[GB:GB + no].view(B, T, Hq, D), lb[GB:GB + nl].view(B, T, Hq), wb[GB:GB + need]
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    e.call(q.to(dev), kp.to(dev), vp.to(dev), bt.to(dev), sl, ks.to(dev), vs.to(dev), o, lse, ws if need else None)
    torch.cuda.synchronize()
    for buf, n in ((ob, no), (lb, nl)):
        assert bool((buf[:GB] == 777.0).all()) and bool((buf[GB + n:] == 777.0).all())
    assert bool((wb[:GB] == 0xA5).all()) and bool((wb[GB + need:] == 0xA5).all())
    e.check(o.cpu(), lse.cpu(), q, kp, vp, bt, lens, ks, vs, "guarded D=%d %s" % (D, shape))
    auto = e.run(q, kp, vp, bt, lens, ks, vs)  # no workspace given
    assert torch.equal(auto[0], o.cpu()) and torch.equal(auto[1], lse.cpu())
    nolse = e.run(q, kp, vp, bt, lens, ks, vs, want_lse=False)
    assert torch.equal(nolse[0], auto[0])


# ---- 10: the serving chain


def check_appended(gk, gv, qo, before_k, ref, bt, lens, T, page, ks, what):
    """The rules of check_appended of tests/test_gpu_fa2_decode_paged_fp8.py: V bytes equal the reference chain's; every K byte outside the
    step's live rows as before the step; every element of the live K rows within fp8_kv_reference.bound of the fp64 rotation (+-448 exactly
    beyond the clamp); q_out within kv_append_reference.bound."""
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
    print("%s: K worst error / bound %.4f, q_out %.4f" % (what, worst, qworst))
    assert worst <= 1.0 and qworst <= 1.0, (what, worst, qworst)


def serving_chain(D):
    """kv_append_paged_fp8 (rope "half") then attention on one stream, page 16, Hkv = 2, G = 4: a 40-token prompt in chunks of 17 and 23 through
    fa2_prefill_paged_fp8, then three steps of T = 2 through fa2_decode_paged_multi_fp8. The reference chain appends with ref_append_fp8 from
    the pools of the previous reference step; after every step the GPU pools are checked against it, and the attention of the step is held to
    the reference on those checked pools."""
    import cuda_learn_notes_amd as pkg
    B, Hkv, G, page, mp = 2, 2, 4, 16, 4
    Hq, dev = Hkv * G, "cuda"
    g = torch.Generator().manual_seed(23 + D)
    P = B * mp + 3
    bt = torch.randperm(P, generator=g)[:B * mp].view(B, mp).to(torch.int32)
    ks, vs = scales_for(Hkv, "k") * 1.3, scales_for(Hkv, "v") * 1.3
    table = pkg.kv_append_rope_table(mp * page, D)
    kp, vp = ((torch.randint(0, 0x7F, (P, Hkv, page, D), generator=g) | (torch.randint(0, 2, (P, Hkv, page, D), generator=g) << 7))
              .to(torch.uint8).view(f8.F8) for _ in range(2))  # the history in front of the start lengths: any codes but the NaN ones
    kd, vd, bd, ksd, vsd, td = (t.to(dev) for t in (kp, vp, bt, ks, vs, table))
    rk, rv, gk_before = kp, vp, kp
    lens = [0, 14]
    pre, mul = Entry("prefill"), Entry("multi")
    for s, (e, T) in enumerate(((pre, 17), (pre, 23), (mul, 2), (mul, 2), (mul, 2))):
        kn, vn = (torch.randn(B, T, Hkv, D, generator=g).half() for _ in range(2))
        q = torch.randn(B, T, Hq, D, generator=g).half()
        lens = [n + T for n in lens]  # the lengths count the new tokens
        assert max(lens) <= mp * page
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        qo = torch.full(q.shape, float("nan"), dtype=torch.half, device=dev)
        pkg.kv_append_paged_fp8(kn.to(dev), vn.to(dev), kd, vd, bd, sl, ksd, vsd, q.to(dev), qo, td, "half")
        o = torch.full(q.shape, float("nan"), dtype=torch.half, device=dev)
        lse = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device=dev)
        e.call(qo, kd, vd, bd, sl, ksd, vsd, o, lse)
        torch.cuda.synchronize()
        ref = f8.ref_append_fp8(kn, vn, rk, rv, bt, lens, ks, vs, q, table, 1)
        assert len(ref.live) == B * T
        what = "chain D=%d step %d (%s, T=%d, lens %s)" % (D, s, e.name, T, lens)
        check_appended(kd.cpu(), vd.cpu(), qo.cpu(), gk_before, ref, bt, lens, T, page, ks, what)
        rk, rv, gk_before = ref.k_pages, ref.v_pages, kd.cpu()
        e.check(o.cpu(), lse.cpu(), qo.cpu(), kd.cpu(), vd.cpu(), bt, lens, ks, vs, what)
    assert lens == [46, 60] and not torch.equal(bits(rk), bits(kp))


# ---- 11: graph replay


def graph_replay(e, D, T):
    """Append plus attention (and for a split plan the merge) captured once on one stream; lengths, table, scales, pools, new rows and q changed
    in place; the replay equals the eager step on the same device state bit for bit, and the reference."""
    import cuda_learn_notes_amd as pkg
    B, Hkv, Hq, page, mp = 2, 2, 8, 16, 64
    shape = (B, Hkv, Hq // Hkv, page, mp, T)
    need = e.need(shape, D)
    assert need > 0 or not e.multi
    _, k8, v8, ks, vs, _, _ = problem(shape, D)
    Nmax, dev = page * mp, "cuda"
    g = torch.Generator().manual_seed(17 + D)
    table = pkg.kv_append_rope_table(Nmax, D)
    state = []
    for i, lens in enumerate(([100, Nmax], [900, 513])):
        kp, vp, bt = f8.make_pool(k8, v8, page, [Nmax] * B, seed=i + 1)  # both pools hold every page of both sequences
        kn, vn = (torch.randn(B, T, Hkv, D, generator=g).half() for _ in range(2))
        q = torch.randn(B, T, Hq, D, generator=g).half()
        state.append((kp, vp, bt, kn, vn, q, lens, ks * (1 + i), vs * (1 + 0.5 * i)))
    assert state[0][0].shape == state[1][0].shape and not torch.equal(state[0][2], state[1][2])
    kp, vp, bt, kn, vn, q, lens, s_k, s_v = state[0]
    kd, vd, bd, knd, vnd, qd, ksd, vsd, td = (t.to(dev).clone() for t in (kp, vp, bt, kn, vn, q, s_k, s_v, table))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    qo, og = torch.zeros_like(qd), torch.zeros_like(qd)
    lg = torch.zeros(B, T, Hq, dtype=torch.float32, device=dev)

    def step(kpool, vpool, q_out, o, lse):
        pkg.kv_append_paged_fp8(knd, vnd, kpool, vpool, bd, sl, ksd, vsd, qd, q_out, td, "half")
        e.call(q_out, kpool, vpool, bd, sl, ksd, vsd, o, lse, ws)

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
    check_appended(kd.cpu(), vd.cpu(), qo.cpu(), kp, ref, bt, lens, T, page, s_k, "graph replay %s D=%d" % (e.kind, D))
    e.check(og.cpu(), lg.cpu(), qo.cpu(), kd.cpu(), vd.cpu(), bt, lens, s_k, s_v, "graph replay D=%d" % D)


# ---- 12: Python argument errors


def python_argument_errors(e, T):
    import cuda_learn_notes_amd as pkg
    import pytest
    dev = "cuda"
    B, Hkv, G, page, mp, D = 2, 2, 4, 16, 64, 64
    Hq, P = Hkv * G, 200
    q = torch.zeros(B, T, Hq, D, dtype=torch.half, device=dev)
    kp = torch.zeros(P, Hkv, page, D, dtype=torch.uint8, device=dev).view(f8.F8)
    vp = kp.clone()
    bt = torch.zeros(B, mp, dtype=torch.int32, device=dev)
    sl = torch.tensor([5, 9], dtype=torch.int32, device=dev)
    ks, vs = torch.ones(Hkv, device=dev), torch.ones(Hkv, device=dev)
    o = torch.empty_like(q)
    f = getattr(pkg, e.name)
    f16 = getattr(pkg, e.fp16_name)
    f(q, kp, vp, bt, sl, ks, vs, o)
    kh, vh = kp.view(torch.uint8).half(), vp.view(torch.uint8).half()
    f16(q, kh, vh, bt, sl, o)
    bad = [
        lambda: f(q, kh, vh, bt, sl, ks, vs, o),                                                    # fp16 pools: the other entry's
        lambda: f16(q, kp, vp, bt, sl, o),                                                          # FP8 pools to the fp16 entry
        lambda: f(q, kp.view(torch.uint8), vp, bt, sl, ks, vs, o),                                  # bytes that are no e4m3 tensor
        lambda: f(q, kp, vp.view(torch.float8_e5m2), bt, sl, ks, vs, o),
        lambda: f(q.float(), kp, vp, bt, sl, ks, vs, o),
        lambda: f(q[:, 0].contiguous(), kp, vp, bt, sl, ks, vs, o[:, 0].contiguous()),              # q without the T dimension
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
        lambda: f(q, kp, vp, bt, sl, ks, vs, o[:, :, :2].contiguous()),
        lambda: f(q, kp, vp, bt, sl, ks, vs, o, lse=torch.empty(B, T, Hq + 1, dtype=torch.float32, device=dev)),
        lambda: f(q, kp, vp, bt, sl, ks, vs, o, lse=torch.empty(B, T, Hq, dtype=torch.half, device=dev)),
        lambda: f(q, kp, vp, bt, sl, ks, vs, q),                                                    # o is an input
    ]
    if e.multi:
        need = pkg.fa2_decode_paged_multi_fp8_plan(B, T, Hq, Hkv, mp, page, D)[2]
        assert need > 0
        bad.append(lambda: f(q, kp, vp, bt, sl, ks, vs, o, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev)))  # short workspace
        q9 = torch.zeros(B, 9, Hq, D, dtype=torch.half, device=dev)
        with pytest.raises(RuntimeError, match=r"T 9 not supported"):
            f(q9, kp, vp, bt, sl, ks, vs, torch.empty_like(q9))
    for i, g in enumerate(bad):
        with pytest.raises(RuntimeError):
            g()
        print("argument error %d raised" % i)
    q6 = torch.zeros(B, T, 6, D, dtype=torch.half, device=dev)
    with pytest.raises(RuntimeError, match=e.name + ": group size 3"):
        f(q6, kp, vp, bt, sl, ks, vs, torch.empty_like(q6))
    kp48 = torch.zeros(P, Hkv, 48, D, dtype=torch.uint8, device=dev).view(f8.F8)
    with pytest.raises(RuntimeError, match=e.name + ": page size 48"):
        f(q, kp48, kp48.clone(), bt, sl, ks, vs, o)
    q96 = torch.zeros(B, T, Hq, 96, dtype=torch.half, device=dev)
    kp96 = torch.zeros(P, Hkv, page, 96, dtype=torch.uint8, device=dev).view(f8.F8)
    with pytest.raises(RuntimeError, match=e.name + ": headdim 96"):
        f(q96, kp96, kp96.clone(), bt, sl, ks, vs, torch.empty_like(q96))
