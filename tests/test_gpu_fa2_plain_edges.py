"""GPU: the plain FlashAttention-2 forward names (flash_attn_mma_stages_*, the family bench.py runs) on every kernel their planner picks --
fa2_fwd_splitkv, fa2_fwd_v2 at 2 / 4 / 8 waves with V and V^T, fa2_fwd_m16x / m16 / m16x64r, fa2_fwd_pair2 (D 320 / 384 / 512) and fa2_fwd_dw4
(D 640 / 768 / 1024) -- where the whole-tensor parity tests of tests/test_gpu_flash_attn.py do not look. Over the table of
tests/fa_plain_cases.py (proven on the CPU by tests/test_fa2_plain_edges_surface.py): (a) parity per flattened head on Gaussian inputs and
on a creeping maximum with a late dominant key and an early spike in every head, (b) a one-hot softmax whose answer V[pi] is known exactly
(target scores up to 510 nats), (c) guard bands around every operand, (d) head independence and head order bit for bit (both block-id -> head
maps of every kernel), (e) all 28 names, grouped by the kernel their plan names, agreeing on every bit; then N = 8192 at six head dims.
Every output buffer starts as NaN; stages 1 and 2 must agree on every bit everywhere. Reference: oracle.attention_fp64. Bounds: the
project's rules, unchanged -- fa_tol (plain names, D <= 128) and fa_tol_f32 (D >= 256, split_kv, *_acc_f32) of tests/fa_reference.py on
each head's own max|O_ref|; 2^-10 |V[pi]| + 1e-5 per element for (b), the rule of test_onehot_attention. Every case prints
`error / bound` before it asserts (pytest -s); the figures of one MI355X run are profiles/r36_fa2_plain_edge_tests.log."""
import pytest
import torch

import fa_plain_cases as fc
import fa_reference as far

pytestmark = pytest.mark.gpu

ROWS = pytest.mark.parametrize("row", fc.TABLE, ids=fc.row_id)


@pytest.fixture(scope="module")
def fa(built, dev):
    return built.flash_attn_lib()


@pytest.fixture(scope="module")
def vt_names(built):
    return built.manifest.FA_V_TRANSPOSED


def seed_of(row, salt):
    kind, name, B, H, N, D = row
    return salt + 7 * B + 13 * H + N + 3 * D + (1 if name == fc.VT else 0)


def laid_out(name, v, vt_names):
    return v.transpose(-2, -1).contiguous() if name in vt_names else v


def run(fa, name, q, k, v, stages, o=None):
    """O of `name` on device tensors (v already in the layout the name takes), written into a buffer that starts as NaN."""
    o = torch.full_like(q, float("nan")) if o is None else o
    getattr(fa, name)(q, k, v, o, stages)
    torch.cuda.synchronize()
    return o


def run_both(fa, name, q, k, v, what):
    o2, o1 = run(fa, name, q, k, v, 2), run(fa, name, q, k, v, 1)
    assert bool(torch.isfinite(o2).all()), what
    assert torch.equal(o1, o2), (what, "stages 1 and 2 differ")
    return o2


def report(what, part, err, bound):
    print("%-40s %-14s %.3e / %.3e = %.3f%s" % (what, part, err, bound, err / bound, "  OVER_HALF" if err > 0.5 * bound else ""))


def hold(what, part, o, ref, rule):
    err, bound, ratio = fc.head_errors(o, ref, rule)
    report(what, part, err, bound)
    assert ratio <= 1.0, (what, part, err, bound)


_GAUSS = {}


def gauss_case(row, oracle, dev):
    """(q, k, v on the device, the fp64 reference per flattened head) of a row's Gaussian inputs: computed once, shared by (a), (c), (d), (e)."""
    if row not in _GAUSS:
        q, k, v = fc.gauss(*row[2:], seed=seed_of(row, 100))
        _GAUSS[row] = tuple(t.to(dev) for t in (q, k, v)) + (fc.ref_heads(oracle, q, k, v),)
    return _GAUSS[row]


# ---- a. parity per head


@ROWS
def test_parity_per_head(fa, dev, oracle, vt_names, row):
    kind, name, B, H, N, D = row
    what, rule = fc.row_id(row), fc.tol_rule(name, D)
    q, k, v, ref = gauss_case(row, oracle, dev)
    hold(what, "gauss", run_both(fa, name, q, k, laid_out(name, v, vt_names), what), ref, rule)
    q, k, v = fc.spiked(B, H, N, D, seed=seed_of(row, 200))
    ref = fc.ref_heads(oracle, q, k, v)
    q, k, v = (t.to(dev) for t in (q, k, v))
    hold(what, "spiked", run_both(fa, name, q, k, laid_out(name, v, vt_names), what), ref, rule)


# ---- b. one-hot attention: O = V[pi]


@ROWS
def test_onehot_exact_answers(fa, dev, vt_names, row):
    kind, name, B, H, N, D = row
    what = fc.row_id(row)
    q, k, v, vp = fc.onehot(B, H, N, D, seed=seed_of(row, 300) * 1000)
    q, k, v, vp = (t.to(dev) for t in (q, k, v, vp))
    o = run_both(fa, name, q, k, laid_out(name, v, vt_names), what)
    diff, bound = (o.double() - vp.double()).abs(), 2.0 ** -10 * vp.double().abs() + 1e-5
    worst = (diff / bound).argmax()
    report(what, "onehot", diff.flatten()[worst].item(), bound.flatten()[worst].item())
    assert bool((diff <= bound).all()), (what, (diff - bound).max().item())


# ---- c. guard bands


@ROWS
def test_guard_bands(fa, dev, oracle, vt_names, row):
    kind, name, B, H, N, D = row
    what = fc.row_id(row)
    q, k, v, _ = gauss_case(row, oracle, dev)
    v = laid_out(name, v, vt_names)
    plain = run_both(fa, name, q, k, v, what)
    gq, gk, gv = (far.guarded(t.shape, t.dtype, t)[1] for t in (q, k, v))
    for stages in (2, 1):
        buf, go = far.guarded(q.shape, torch.float16)
        assert bool(torch.isfinite(buf[0]).all()) and bool(torch.isfinite(buf[-1]).all()) and bool(torch.isnan(go).all())
        keep = far.pads(buf)
        run(fa, name, gq, gk, gv, stages, o=go)
        assert torch.equal(far.pads(buf), keep), (what, stages, "pad overwritten")
        assert bool(torch.isfinite(go).all()), (what, stages)
        assert torch.equal(go, plain), (what, stages, "payload differs from the run on ordinary allocations")
    print("%-40s pads intact, payloads bit-identical" % what)


# ---- d. heads


@ROWS
def test_heads_are_independent_and_in_order(fa, dev, oracle, vt_names, row):
    kind, name, B, H, N, D = row
    what, rule, n = fc.row_id(row), fc.tol_rule(name, D), B * H
    q, k, v, _ = gauss_case(row, oracle, dev)
    base = run(fa, name, q, k, laid_out(name, v, vt_names), 2).view(n, N, D)
    g = torch.Generator().manual_seed(seed_of(row, 400))
    for h in (0, n // 2, n - 1):
        new = [torch.randn(N, D, generator=g).half() for _ in range(3)]
        q2, k2, v2 = (t.clone() for t in (q, k, v))
        for t, x in zip((q2, k2, v2), new):
            t.view(n, N, D)[h] = x.to(dev)
        o = run(fa, name, q2, k2, laid_out(name, v2, vt_names), 2).view(n, N, D)
        others = [i for i in range(n) if i != h]
        assert torch.equal(o[others], base[others]), (what, h, "another head changed")
        assert not torch.equal(o[h], base[h]), (what, h)
        hold(what, "head %d" % h, o[h:h + 1], fc.ref_heads(oracle, *(x[None, None] for x in new)), rule)
    p = fc.derangement(n, seed_of(row, 500)).to(dev)
    qp, kp, vp = (t.view(n, N, D)[p].view(B, H, N, D) for t in (q, k, v))
    o = run(fa, name, qp, kp, laid_out(name, vp, vt_names), 2).view(n, N, D)
    assert torch.equal(o, base[p]), (what, "permuted heads")
    print("%-40s heads independent, permutation of %d heads kept every bit" % (what, n))


# ---- e. the names agree


@ROWS
def test_names_that_share_a_kernel_agree_on_every_bit(fa, built, dev, oracle, vt_names, row):
    kind, _, B, H, N, D = row
    what = fc.row_id(row)
    q, k, v, ref = gauss_case(row, oracle, dev)
    vs = {False: v, True: laid_out(fc.VT, v, vt_names)}
    names = [e.name for e in built.manifest.entries_of("flash_attn")]
    assert len(names) == 28
    groups, unsupported = {}, []
    for name in names:
        try:
            groups.setdefault(built.manifest.describe(name, (B, H, N, D), 2), []).append(name)
        except ValueError:
            unsupported.append(name)
    for name in unsupported:
        for stages in (1, 2):
            with pytest.raises(ValueError):
                built.manifest.describe(name, (B, H, N, D), stages)
            with pytest.raises(RuntimeError):
                getattr(fa, name)(q, k, vs[name in vt_names], torch.full_like(q, float("nan")), stages)
    assert sum(len(g) for g in groups.values()) + len(unsupported) == 28 and groups, what
    for text, group in groups.items():
        first = run_both(fa, group[0], q, k, vs[group[0] in vt_names], (what, group[0]))
        for name in group[1:]:
            assert (name in vt_names) == (group[0] in vt_names)
            for stages in (2, 1):
                assert torch.equal(run(fa, name, q, k, vs[name in vt_names], stages), first), (what, name, stages, "differs from", group[0])
        hold(what, "%d x %s" % (len(group), text[:text.index("<")][8:]), first, ref, fc.tol_rule(group[0], D))
        assert len({fc.tol_rule(n, D) for n in group}) == 1, group
    print("%-40s %d names in %d kernels, %d unsupported" % (what, 28 - len(unsupported), len(groups), len(unsupported)))


# ---- N = 8192


def rows_reference(q, k, v, r0, rows=128):
    """fp64 attention of query rows [r0, r0 + rows) of every flattened head over all keys: [B H, rows, D]."""
    B, H, N, D = q.shape
    qf, kf, vf = (t.reshape(B * H, N, D).double() for t in (q, k, v))
    s = qf[:, r0:r0 + rows] @ kf.transpose(-1, -2) / D ** 0.5
    return torch.softmax(s, dim=-1) @ vf


@pytest.mark.parametrize("row", fc.LONG, ids=fc.row_id)
def test_long_sequences(fa, dev, vt_names, row):
    """N = 8192 against the fp64 reference on the first, a middle (4032..4159) and the last block of 128 query rows of both heads; every
    other row finite. The rules' calibration log stops at N = 4096: the measured error / bound of each case is printed."""
    kind, name, B, H, N, D = row
    what, rule = fc.row_id(row), fc.tol_rule(name, D)
    q, k, v = fc.gauss(B, H, N, D, seed=seed_of(row, 600))
    o = run_both(fa, name, q.to(dev), k.to(dev), laid_out(name, v.to(dev), vt_names), what).view(B * H, N, D)
    for r0 in fc.LONG_BLOCKS:
        hold(what, "rows %d.." % r0, o[:, r0:r0 + 128], rows_reference(q, k, v, r0), rule)
