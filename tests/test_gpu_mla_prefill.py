"""GPU: the prompt path of multi-head latent attention -- cuda_learn_notes_amd.fa2_prefill_varlen_mla_bf16, attn_merge_states_bf16 and
kv_gather_paged_mla_bf16 (csrc/flash_attn_prefill_varlen_mla_bf16.*, attn_merge_states_bf16.*, kv_gather_paged_mla_bf16.*) --
against tests/mla_prefill_reference.py (fp64 and the bf16 emulation, anchored to the existing reference by tests/test_mla_prefill_surface.py).
No new tolerance for the attention: O within paged_bf16_reference.o_bound of the emulation, LSE within decode_reference.lse_tol per head, -inf
LSE entries and zero rows exactly (test_gpu_paged_sink_attention.check). The merge: per element 2^-8 |r| + 2^-20 max(|O_a|, |O_b|) of the fp64
merge of the same bf16 inputs (mla_prefill_reference.merge_bound has the derivation). Beyond parity: exact counts at every tile edge, the two
halves of the key, bit equalities -- a sequence alone, a head alone, guard bands, a captured graph -- the chunked chain, and the prefill and the
latent decode against one fp64 reference. Every parity case prints err / bound before it asserts (pytest -s); the last test prints the largest
per group.

Largest err / bound seen on an MI355X: see DESIGN 4.4.18 and profiles/r28_mla_prefill_tests.log."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as dr  # noqa: E402
import mla_prefill_reference as mp  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_edge_cases as ec  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DN, DR, DQ, DV, SCALE = mp.DN, mp.DR, mp.DQ, mp.DV, mp.SCALE
O_FILL, L_FILL = sk.O_FILL, sk.L_FILL
NEG_INF = float("-inf")
bits, fbits, check = sk.bits, sk.fbits, sk.check
RATIOS = {}
DEV = "cuda"


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def filled(shape, dtype):
    if dtype == BF:
        return torch.full(shape, O_FILL, dtype=torch.int16, device=DEV).view(BF)
    return torch.full(shape, L_FILL, dtype=torch.int32, device=DEV).view(torch.float32)


def prefill(q, kv, k_pe, cu_q, cu_k, causal=True, scale=SCALE):
    """(o, lse) on the CPU, pre-filled with the sentinels."""
    o, lse = filled((q.shape[0], q.shape[1], DV), BF), filled(q.shape[:2], torch.float32)
    pkg().fa2_prefill_varlen_mla_bf16(q.to(DEV), kv.to(DEV), k_pe.to(DEV), i32(cu_q), i32(cu_k), scale, o, lse, causal)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def same(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(fbits(a[1]), fbits(b[1]))


def check_rows(got, ref, rows, what):
    """check() on the rows of the sequences."""
    return check(got[0][rows], got[1][rows], ref[0][rows], ref[1][rows], ref[2][rows], what)


# ---------------------------------------------------------------------------------------------------- 1, 3. one sequence

@pytest.mark.parametrize("causal", [True, False], ids=["causal", "non-causal"])
@pytest.mark.parametrize("case", mp.ONE_CASES, ids=lambda c: "T%d+%dxHq%d" % c)
def test_one_sequence(built, dev, case, causal):
    """T at 1, around the 16-row tile, the wave's 32 rows and the 128-row workgroup tile, three tiles; contexts that put the causal edge at
    and around the 64-key step; non-causal: every row sees all L keys, at the same edges."""
    T, ctx, Hq = case
    q, kv, k_pe, cu_q, cu_k = mp.one_case(T, ctx, Hq)
    got = prefill(q, kv, k_pe, cu_q, cu_k, causal)
    ref = mp.prefill(q, kv, k_pe, cu_q, cu_k, SCALE, causal)
    assert bool(torch.isfinite(ref[1]).all())
    group = "prefill, one sequence, " + ("causal" if causal else "non-causal")
    note(group, check(*got, *ref, "mla prefill %s T=%d ctx=%d Hq=%d" % ("causal" if causal else "full", T, ctx, Hq)))


# ---------------------------------------------------------------------------------------------------- 2. packed ragged batch

@pytest.mark.parametrize("causal", [True, False], ids=["causal", "non-causal"])
def test_packed_ragged_batch(built, dev, causal):
    """T = 129, 0, 1, 64, 33 with L = T + 0, 5, 64, 0, 200, and T = 40, 17 with L = 25, 17 (the first 15 rows of the first see no key when
    causal); cu_q[0] = 3 and 5 trailing rows; o and lse sit inside sentinel guard bands; every sequence alone (B = 1) gives the packed bits."""
    Hq = 3
    Ts, Ls = tuple(mp.RAGGED_T + mp.SHORT_T), tuple(mp.RAGGED_L + mp.SHORT_L)
    q, kv, k_pe, cu_q, cu_k = mp.packed_case(Ts, Ls, Hq, seed=1, front=mp.FRONT, back=mp.BACK)
    tq = q.shape[0]
    assert cu_q[0] == 3 and cu_q[-1] + 5 == tq
    big_o, big_l = filled((tq + 4, Hq, DV), BF), filled((tq + 4, Hq), torch.float32)
    pkg().fa2_prefill_varlen_mla_bf16(q.to(DEV), kv.to(DEV), k_pe.to(DEV), i32(cu_q), i32(cu_k), SCALE, big_o[2:tq + 2], big_l[2:tq + 2], causal)
    torch.cuda.synchronize()
    big_o, big_l = big_o.cpu(), big_l.cpu()
    got = (big_o[2:tq + 2], big_l[2:tq + 2])
    seq = slice(cu_q[0], cu_q[-1])
    for sl in (slice(0, 2 + cu_q[0]), slice(2 + cu_q[-1], None)):  # the guard bands and the packed rows of no sequence
        assert bool((bits(big_o[sl]) == O_FILL).all()) and bool((fbits(big_l[sl]) == L_FILL).all())
    ref = mp.prefill(q, kv, k_pe, cu_q, cu_k, SCALE, causal)
    short = slice(cu_q[5], cu_q[5] + 15)
    if causal:
        assert bool((ref[1][short] == NEG_INF).all()) and bool(torch.isfinite(ref[1][cu_q[5] + 15:cu_q[6]]).all())
        assert bool((bits(got[0][short]) == 0).all()) and bool((got[1][short] == NEG_INF).all())
    else:
        assert bool(torch.isfinite(ref[1][seq]).all())
    note("prefill, packed ragged, " + ("causal" if causal else "non-causal"), check_rows(got, ref, seq, "mla prefill packed causal=%d" % causal))
    for b in range(len(Ts)):
        if Ts[b] == 0:
            continue
        rows, keys = slice(cu_q[b], cu_q[b + 1]), slice(cu_k[b], cu_k[b + 1])
        kb, pb = (kv[keys], k_pe[keys]) if Ls[b] else (kv[:1], k_pe[:1])  # total_k >= 1
        one = prefill(q[rows].contiguous(), kb.contiguous(), pb.contiguous(), [0, Ts[b]], [0, Ls[b]], causal)
        assert same(one, (got[0][rows], got[1][rows])), b
    again = prefill(q, kv, k_pe, cu_q, cu_k, causal)  # two calls
    assert same((again[0][seq], again[1][seq]), (got[0][seq], got[1][seq]))


@pytest.mark.parametrize("scale", mp.OTHER_SCALES, ids=["yarn", "quarter"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "non-causal"])
def test_packed_ragged_batch_at_a_scale_that_is_not_the_datas(built, dev, causal, scale):
    """The ragged packed batch at V3's YaRN scale and at SCALE / 4: the reference at SCALE is more than 20 x o_bound away (proven without a
    GPU by tests/test_mla_prefill_surface.py; Q_MULT = 1, the data is standard normal)."""
    q, kv, k_pe, cu_q, cu_k, ref, ref0 = mp.scale_case(causal, scale)
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla prefill scale %.5f causal=%d: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, causal, diff, need))
    assert diff > need
    got = prefill(q, kv, k_pe, cu_q, cu_k, causal, scale=scale)
    note("prefill, another scale", check_rows(got, ref, slice(cu_q[0], cu_q[-1]), "mla prefill packed causal=%d scale=%.5f" % (causal, scale)))


def test_refusals_on_the_device(built, dev):
    """Contiguity is part of the device check; lse = None leaves o's bits."""
    q, kv, k_pe, cu_q, cu_k = mp.one_case(17, 64, 3)
    qd, kd, pd = q.to(DEV), kv.to(DEV), k_pe.to(DEV)
    o = filled((17, 3, DV), BF)
    with pytest.raises(RuntimeError, match="contiguous"):
        pkg().fa2_prefill_varlen_mla_bf16(qd, kd.transpose(0, 1).contiguous().transpose(0, 1), pd, i32(cu_q), i32(cu_k), SCALE, o)
    with pytest.raises(RuntimeError, match="contiguous"):
        pkg().attn_merge_states_bf16(o.transpose(0, 1), torch.zeros(3, 17, device=DEV), o.transpose(0, 1), torch.zeros(3, 17, device=DEV), o.transpose(0, 1))
    assert bool((bits(o.cpu()) == O_FILL).all())
    pkg().fa2_prefill_varlen_mla_bf16(qd, kd, pd, i32(cu_q), i32(cu_k), SCALE, o)
    torch.cuda.synchronize()
    assert torch.equal(bits(o.cpu()), bits(prefill(q, kv, k_pe, cu_q, cu_k)[0]))


# ---------------------------------------------------------------------------------------------------- 4. exact counts

@pytest.mark.parametrize("causal", [True, False], ids=["causal", "non-causal"])
def test_exact_counts(built, dev, causal):
    """q = 0 and v = 1 (k_nope, k_pe random): every weight of a row is 1 / n, so O is exactly 1 and LSE = ln n. Causal: T = 129 rows over L = 129
    keys, row t sees n = t + 1: every n of 1 ... 129, the edges 1, 15, 16, 17, 63, 64, 65, 127, 128, 129 among them, and the same rows behind 64
    keys of context. Non-causal: one sequence per n, T = 33."""
    Hq = 2
    g = torch.Generator().manual_seed(11)
    if causal:
        Ts, Ls = [129, 129], [129, 193]
    else:
        Ts, Ls = [33] * len(mp.COUNT_N), list(mp.COUNT_N)
    cu_q, cu_k = mp.cu_of(Ts), mp.cu_of(Ls)
    q = torch.zeros(cu_q[-1], Hq, DQ, dtype=BF)
    kv = torch.randn(cu_k[-1], Hq, mp.DKV, generator=g).to(BF)
    kv[..., DN:] = 1
    k_pe = torch.randn(cu_k[-1], DR, generator=g).to(BF)
    o, lse = prefill(q, kv, k_pe, cu_q, cu_k, causal)
    worst, seen = 0.0, set()
    for b, (T, L) in enumerate(zip(Ts, Ls)):
        for t, n in enumerate(mp.visible(T, L, causal)):
            row = cu_q[b] + t
            assert n > 0 and bool((o[row] == 1).all()), (b, t, n)
            err, tol = (lse[row].double() - math.log(n)).abs().max().item(), ec.lse_tol_at(n)
            worst = max(worst, err / tol)
            seen.add(n)
            assert err <= tol, (b, t, n, err, tol)
    assert set(mp.COUNT_N) <= seen
    print("mla prefill counts causal=%d: %d distinct n, LSE = ln n within %.4f of the tolerance" % (causal, len(seen), worst))


# ---------------------------------------------------------------------------------------------------- 5. the two halves of the key

def _big(t):
    t = t.clone()
    t[..., 0::2], t[..., 1::2] = 2.0 ** 60, -2.0 ** 60
    return t


def test_the_two_halves_of_the_key(built, dev):
    Hq = 3
    q, kv, k_pe, cu_q, cu_k = mp.packed_case((129, 33), (194, 33), Hq, seed=2)
    # q_pe = 0: k_pe meets zeros
    q1 = q.clone()
    q1[..., DN:] = 0
    a, b = prefill(q1, kv, k_pe * 0, cu_q, cu_k), prefill(q1, kv, _big(k_pe), cu_q, cu_k)
    assert same(a, b)
    note("prefill, q_pe = 0", check(*a, *mp.prefill(q1, kv, k_pe * 0, cu_q, cu_k, SCALE), "mla prefill q_pe=0"))
    # q_nope = 0: k_nope meets zeros; V untouched. The rotary dims alone make the scores: 4 x the usual size, far from uniform
    q2 = q.clone()
    q2[..., :DN] = 0
    q2[..., DN:] = (q2[..., DN:].float() * 4).to(BF)
    kz, kb = kv.clone(), kv.clone()
    kz[..., :DN] = 0
    kb[..., :DN] = _big(kb[..., :DN])
    a, b = prefill(q2, kz, k_pe, cu_q, cu_k), prefill(q2, kb, k_pe, cu_q, cu_k)
    assert same(a, b)
    ref = mp.prefill(q2, kz, k_pe, cu_q, cu_k, SCALE)
    flat = mp.prefill(q2 * 0, kz, k_pe, cu_q, cu_k, SCALE)[0]
    assert float((ref[0] - flat).abs().max()) > 20 * br.o_bound(ref[2], ref[0])  # the uniform average is far outside the bound
    note("prefill, q_nope = 0", check(*a, *ref, "mla prefill q_nope=0"))
    # heads with different k_nope and the one shared k_pe: each matches a single-head call
    base = prefill(q, kv, k_pe, cu_q, cu_k)
    for h in range(Hq):
        one = prefill(q[:, h:h + 1].contiguous(), kv[:, h:h + 1].contiguous(), k_pe, cu_q, cu_k)
        assert same(one, (base[0][:, h:h + 1].contiguous(), base[1][:, h:h + 1].contiguous())), h


# ---------------------------------------------------------------------------------------------------- 6. merge

def run_merge(o_a, lse_a, o_b, lse_b, in_place=False, with_lse=True):
    oa, la, ob, lb = (t.to(DEV) for t in (o_a, lse_a, o_b, lse_b))
    o = oa if in_place else filled(tuple(o_a.shape), BF)
    lse = None if not with_lse else la if in_place else filled(tuple(lse_a.shape), torch.float32)
    pkg().attn_merge_states_bf16(oa, la, ob, lb, o, lse)
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(bits(oa.cpu()), bits(o_a)) and torch.equal(fbits(la.cpu()), fbits(lse_a))
    assert torch.equal(bits(ob.cpu()), bits(o_b)) and torch.equal(fbits(lb.cpu()), fbits(lse_b))
    return o.cpu(), (lse.cpu() if lse is not None else None)


@pytest.mark.parametrize("rows", mp.MERGE_ROWS)
@pytest.mark.parametrize("D", mp.MERGE_D)
def test_merge(built, dev, D, rows):
    g = torch.Generator().manual_seed(D + rows)
    o_a, o_b = (torch.randn(rows, D, generator=g).to(BF) for _ in range(2))
    lse_a, lse_b = (torch.randn(rows, generator=g) * 3 for _ in range(2))
    if rows > 8:  # one side without a key, the other side without, both
        lse_a[3], lse_b[5], lse_a[7], lse_b[7] = NEG_INF, NEG_INF, NEG_INF, NEG_INF
        lse_b[9] = lse_a[9] + 40.0  # a weight of e^-40 against the other
    ro, rl = mp.merge(o_a, lse_a, o_b, lse_b)
    o, lse = run_merge(o_a, lse_a, o_b, lse_b)
    ratio = float(((o.double() - ro).abs() / mp.merge_bound(ro, o_a, o_b).clamp(min=1e-300)).max())
    fin = torch.isfinite(rl)
    el = float((lse.double()[fin] - rl[fin]).abs().max()) if bool(fin.any()) else 0.0
    print("merge D=%d rows=%d: O err / bound %.4f, LSE err %.3e / tol %.3e" % (D, rows, ratio, el, dr.lse_tol(rl)))
    note("merge", ratio)
    assert ratio <= 1.0 and el <= dr.lse_tol(rl) and torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == NEG_INF).all())
    if rows > 8:
        assert bool((bits(o[7]) == 0).all()) and lse[7] == NEG_INF
        assert torch.equal(bits(o[3]), bits(o_b[3])) and torch.equal(bits(o[5]), bits(o_a[5])) and lse[3] == lse_b[3] and lse[5] == lse_a[5]
    # in place, and without lse
    oi, li = run_merge(o_a, lse_a, o_b, lse_b, in_place=True)
    assert torch.equal(bits(oi), bits(o)) and torch.equal(fbits(li), fbits(lse))
    on, none = run_merge(o_a, lse_a, o_b, lse_b, with_lse=False)
    assert none is None and torch.equal(bits(on), bits(o))
    # guard bands
    big_o, big_l = filled((rows + 2, D), BF), filled((rows + 2,), torch.float32)
    pkg().attn_merge_states_bf16(o_a.to(DEV), lse_a.to(DEV), o_b.to(DEV), lse_b.to(DEV), big_o[1:rows + 1], big_l[1:rows + 1])
    torch.cuda.synchronize()
    big_o, big_l = big_o.cpu(), big_l.cpu()
    assert torch.equal(bits(big_o[1:rows + 1]), bits(o)) and torch.equal(fbits(big_l[1:rows + 1]), fbits(lse))
    for edge in (0, rows + 1):
        assert bool((bits(big_o[edge]) == O_FILL).all()) and int(fbits(big_l[edge])) == L_FILL


@pytest.mark.parametrize("D", mp.MERGE_D)
def test_merge_exact_cases(built, dev, D):
    rows = 257
    g = torch.Generator().manual_seed(D)
    o_a = torch.randn(rows, D, generator=g).to(BF)
    lse_a = torch.randn(rows, generator=g) * 3
    ninf = torch.full((rows,), NEG_INF)
    nan = torch.full((rows, D), float("nan")).to(BF)
    o, lse = run_merge(o_a, lse_a, nan, ninf)       # lse_b = -inf with o_b = NaN: the a side, bit for bit
    assert torch.equal(bits(o), bits(o_a)) and torch.equal(fbits(lse), fbits(lse_a))
    o, lse = run_merge(nan, ninf, o_a, lse_a)       # ... and the other way round
    assert torch.equal(bits(o), bits(o_a)) and torch.equal(fbits(lse), fbits(lse_a))
    o, lse = run_merge(nan, ninf, nan, ninf)        # both -inf
    assert bool((bits(o) == 0).all()) and bool((lse == NEG_INF).all())
    o, lse = run_merge(o_a, lse_a, o_a.clone(), lse_a.clone())  # identical states
    assert torch.equal(bits(o), bits(o_a))
    want = lse_a.double() + math.log(2.0)
    assert float((lse.double() - want).abs().max()) <= dr.lse_tol(want)


# ---------------------------------------------------------------------------------------------------- 7. chunked chain

@pytest.mark.parametrize("C", mp.CHAIN_C)
def test_chunked_chain(built, dev, C):
    """Keys [0, C) non-causal and keys [C, L) causal, merged, against the fp64 reference of the one causal call over all keys: within o_bound +
    2^-8 max(|O_a|, |O_b|) -- each partial carries one extra rounding to bf16 and the weights sum to 1."""
    T, Hq = mp.CHAIN_T, 3
    L = C + T
    q, kv, k_pe, cu_q, cu_k = mp.one_case(T, C, Hq)
    ctx = prefill(q, kv[:C].contiguous(), k_pe[:C].contiguous(), [0, T], [0, C], causal=False)
    new = prefill(q, kv[C:].contiguous(), k_pe[C:].contiguous(), [0, T], [0, T], causal=True)
    o, lse = run_merge(new[0], new[1], ctx[0], ctx[1])
    ro, rl, emul = mp.prefill(q, kv, k_pe, [0, T], [0, L], SCALE, causal=True)
    bound = br.o_bound(emul, ro) + 2.0 ** -8 * float(torch.maximum(new[0].double().abs(), ctx[0].double().abs()).max())
    eo = float((o.double() - ro).abs().max())
    el = float((lse.double() - rl).abs().max())
    print("mla chunked chain C=%d T=%d: O err %.3e / bound %.3e = %.4f, LSE err %.3e / tol %.3e" % (C, T, eo, bound, eo / bound, el, dr.lse_tol(rl)))
    note("chunked chain", eo / bound)
    assert eo <= bound and el <= dr.lse_tol(rl)


# ---------------------------------------------------------------------------------------------------- 8. prefill and decode agree

def _latent_problem():
    """Hq = 4, T = 5, L = 100, one sequence: latent rows [c 512 | k_pe 64] whose up-projection is a selection -- head h takes latent dims
    128 h ... 128 h + 127 as k_nope and as v -- so it is exact in bf16 and the absorbed q is q_nope scattered into 512 dims."""
    Hq, T, L, page = 4, 5, 100, 16
    g = torch.Generator().manual_seed(8)
    c_rows = (torch.randn(L, ml.DC, generator=g) * 0.5).to(BF)
    pe = (torch.randn(L, DR, generator=g) * 0.5).to(BF)
    q = torch.randn(T, Hq, DQ, generator=g).to(BF)
    return Hq, T, L, page, c_rows, pe, q


def test_prefill_and_decode_agree(built, dev):
    c = pkg()
    Hq, T, L, page, c_rows, pe, q = _latent_problem()
    max_pages = 8
    # append the latent rows through the library: an empty cache, then all L tokens at once
    dense = torch.zeros(1, max_pages * page, ml.DK, dtype=BF)
    pool0, bt = ml.make_pool(dense, page, [L], seed=4)
    pool = pool0.to(DEV)
    c.kv_append_paged_mla_bf16(c_rows.to(DEV), pe.to(DEV), pool, bt.to(DEV), i32([L]), i32([0, L]))
    # gather them back: bit for bit the reference's gather
    packed = filled((L, ml.DK), BF)
    c.kv_gather_paged_mla_bf16(pool, bt.to(DEV), i32([0, L]), packed)
    torch.cuda.synchronize()
    packed = packed.cpu()
    assert torch.equal(bits(packed), bits(ml.gather(pool.cpu(), bt, [L])[0, :L]))
    assert torch.equal(bits(packed[:, :ml.DC]), bits(c_rows)) and torch.equal(bits(packed[:, ml.DC:]), bits(pe))
    # the up-projection (the caller's kv_b_proj), here a selection: kv [L, Hq, 256] = [k_nope_h | v_h], both latent dims 128 h ...
    lat = packed[:, :ml.DC].reshape(L, Hq, DN)
    kv = torch.cat([lat, lat], dim=-1).contiguous()
    k_pe = packed[:, ml.DC:].contiguous()
    ref = mp.prefill(q, kv, k_pe, [0, T], [0, L], SCALE)
    got = prefill(q, kv, k_pe, [0, T], [0, L])
    note("prefill against decode", check(*got, *ref, "mla prefill on the gathered rows"))
    # the absorbed q of the decode: q_nope scattered into head h's 128 latent dims
    qa = torch.zeros(1, T, Hq, ml.DK, dtype=BF)
    for h in range(Hq):
        qa[0, :, h, DN * h:DN * (h + 1)] = q[:, h, :DN]
    qa[0, :, :, ml.DC:] = q[:, :, DN:]
    o = filled((1, T, Hq, ml.DC), BF)
    lse = filled((1, T, Hq), torch.float32)
    c.fa2_decode_paged_mla_bf16(qa.to(DEV), pool, bt.to(DEV), i32([L]), SCALE, o, lse)
    torch.cuda.synchronize()
    o, lse = o.cpu(), lse.cpu()
    dec_o = torch.stack([o[0, :, h, DN * h:DN * (h + 1)] for h in range(Hq)], dim=1)
    dref = ml.decode(qa, pool.cpu(), bt, [L], SCALE)
    dec_e = torch.stack([dref[2][0, :, h, DN * h:DN * (h + 1)] for h in range(Hq)], dim=1)
    assert float((torch.stack([dref[0][0, :, h, DN * h:DN * (h + 1)] for h in range(Hq)], dim=1) - ref[0]).abs().max()) < 1e-12  # one reference
    assert float((dref[1][0] - ref[1]).abs().max()) < 1e-12
    note("decode against prefill", check(dec_o, lse[0], ref[0], ref[1], dec_e, "mla decode, its dims 128 h ..., against the prefill's reference"))


# ---------------------------------------------------------------------------------------------------- 9. gather

GATHER_LENS, GATHER_NMAX = [100, 37, 256], 256


def _gather_problem(page):
    g = torch.Generator().manual_seed(page)
    dense = torch.randn(len(GATHER_LENS), GATHER_NMAX, ml.DK, generator=g).to(BF)
    return ml.make_pool(dense, page, GATHER_LENS, seed=page)


@pytest.mark.parametrize("starts", [None, [0, 7, 64]], ids=["from-0", "starts"])
@pytest.mark.parametrize("page", [16, 256])
def test_gather(built, dev, page, starts):
    """Cache lengths 100, 37, 256 in tables of 256 rows; chunks [start, start + n): whole caches, a chunk inside a page, one crossing page
    edges, and (with starts) one that reaches 20 rows past max_pages page: zeros. Pages no live table entry names hold 2^100 and never appear."""
    pool, bt = _gather_problem(page)
    st = starts or [0, 0, 0]
    counts = [100, 30, 256 - st[2] + (20 if starts else 0)]
    front, back = 3, 4
    cu = mp.cu_of(counts, front)
    total = cu[-1] + back
    out = filled((total + 2, ml.DK), BF)
    pkg().kv_gather_paged_mla_bf16(pool.to(DEV), bt.to(DEV), i32(cu), out[1:total + 1], None if starts is None else i32(st))
    torch.cuda.synchronize()
    out = out.cpu()
    dense = ml.gather(pool, bt, GATHER_LENS)
    for b, n in enumerate(counts):
        got = out[1 + cu[b]:1 + cu[b + 1]]
        inside = min(n, GATHER_NMAX - st[b])
        assert torch.equal(bits(got[:inside]), bits(dense[b, st[b]:st[b] + inside])), b
        assert bool((bits(got[inside:]) == 0).all()), b
        live = min(max(GATHER_LENS[b] - st[b], 0), n)  # rows inside the cache's length: never the filler
        assert not bool((got[:live].float().abs() >= ml.FILL).any()), b
    assert bool((bits(out[:1 + cu[0]]) == O_FILL).all()) and bool((bits(out[1 + cu[-1]:]) == O_FILL).all())
    if starts:
        assert counts[2] > GATHER_NMAX - st[2]


# ---------------------------------------------------------------------------------------------------- 10. a captured graph

def test_a_captured_graph_of_gather_prefill_and_merge_replays_the_eager_bits(built, dev):
    """A chunked step: the context chunk gathered out of the pool and up-projected by selection, attended to non-causally, the new tokens
    causally, the two merged in place. Eager, then the same calls captured in a graph and replayed on fresh buffers."""
    c = pkg()
    Hq, T, C, page = 4, 33, 100, 16
    g = torch.Generator().manual_seed(10)
    dense = (torch.randn(1, 128, ml.DK, generator=g) * 0.5).to(BF)
    pool, bt = ml.make_pool(dense, page, [C], seed=6)
    q = torch.randn(T, Hq, DQ, generator=g).to(BF)
    kv_new = torch.randn(T, Hq, mp.DKV, generator=g).to(BF)
    pe_new = torch.randn(T, DR, generator=g).to(BF)
    fixed = tuple(t.to(DEV) for t in (pool, bt, q, kv_new, pe_new)) + (i32([0, C]), i32([0, T]))

    def buffers():
        return (filled((C, ml.DK), BF), torch.empty(C, Hq, mp.DKV, dtype=BF, device=DEV), torch.empty(C, DR, dtype=BF, device=DEV),
                filled((T, Hq, DV), BF), filled((T, Hq), torch.float32), filled((T, Hq, DV), BF), filled((T, Hq), torch.float32),
                filled((T, Hq, DV), BF), filled((T, Hq), torch.float32))

    def step(packed, kv_ctx, pe_ctx, o, lse, o_new, l_new, o_ctx, l_ctx):
        pl, btd, qd, kvn, pen, cu_c, cu_t = fixed
        c.kv_gather_paged_mla_bf16(pl, btd, cu_c, packed)
        lat = packed[:, :ml.DC].unflatten(1, (Hq, DN))  # the caller's kv_b_proj, here a selection
        kv_ctx[..., :DN].copy_(lat)
        kv_ctx[..., DN:].copy_(lat)
        pe_ctx.copy_(packed[:, ml.DC:])
        c.fa2_prefill_varlen_mla_bf16(qd, kv_ctx, pe_ctx, cu_t, cu_c, SCALE, o_ctx, l_ctx, False)
        c.fa2_prefill_varlen_mla_bf16(qd, kvn, pen, cu_t, cu_t, SCALE, o_new, l_new, True)
        c.attn_merge_states_bf16(o_new, l_new, o_ctx, l_ctx, o, lse)

    eager = buffers()
    step(*eager)
    torch.cuda.synchronize()
    o, lse = eager[3].cpu(), eager[4].cpu()
    lat = dense[0, :C, :ml.DC].reshape(C, Hq, DN)
    kv_all = torch.cat([torch.cat([lat, lat], dim=-1), kv_new], dim=0)
    pe_all = torch.cat([dense[0, :C, ml.DC:], pe_new], dim=0)
    ro, rl, emul = mp.prefill(q, kv_all, pe_all, [0, T], [0, C + T], SCALE)
    bound = br.o_bound(emul, ro) + 2.0 ** -8 * float(torch.maximum(eager[5].cpu().double().abs(), eager[7].cpu().double().abs()).max())
    eo = float((o.double() - ro).abs().max())
    print("mla chunked step through the pool: O err %.3e / bound %.3e = %.4f" % (eo, bound, eo / bound))
    note("chunked chain", eo / bound)
    assert eo <= bound and float((lse.double() - rl).abs().max()) <= dr.lse_tol(rl)
    bufs = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(*bufs)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("packed", "kv", "k_pe", "o"), bufs[:4], eager[:4]):
        assert torch.equal(bits(a.cpu()), bits(b.cpu())), name
    assert torch.equal(fbits(bufs[4].cpu()), fbits(eager[4].cpu()))


def test_zz_summary_of_error_over_bound(built, dev):
    """The RATIOS table: the largest err / bound of every group of parity cases of this file. Not an assertion of its own --
    every case asserted err <= bound where it ran."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-40s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
