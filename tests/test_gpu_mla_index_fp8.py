"""GPU: the DSA indexer's FP8 cache -- cuda_learn_notes_amd.kv_append_paged_index_bf16_fp8 and mla_index_logits_paged_bf16_fp8
(csrc/kv_append_paged_index_bf16_fp8.*, csrc/mla_index_logits_paged_bf16_fp8.*) -- against tests/mla_index_fp8_reference.py.
The append: torch.equal on every pool byte against the CPU reference in the kernel's fp32 operations, guard pages around the pool included.
The logits: within the derived bound 2^-23 (128 + 64 + 3) A of the fp64 reference on the dequantised pool, bit-exact where the answer is
exact and there equal to the bf16 entry on the same codes, nothing written at or past vis or outside the tensor, nothing read behind the
lengths (0x7F code bytes and NaN scales in every unlisted slot and page). Then order independence and the chain of a V3.2 step on e4m3
caches, eager and captured. Every parity case prints err / bound before it asserts (pytest -s); the last test prints the largest per group.
tests/test_mla_index_fp8_surface.py proves on the CPU that every parity case here would notice a wrong scale or a misplaced ReLU.

Largest err / bound seen on an MI355X: see DESIGN 4.4.24."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mla_index_fp8_reference as x8  # noqa: E402
import mla_index_reference as ix  # noqa: E402
import test_gpu_mla_index as gi  # noqa: E402
import test_gpu_paged_mla_sparse_fp8 as t8  # noqa: E402

pytestmark = pytest.mark.gpu

BF, U8, DEV = torch.bfloat16, torch.uint8, "cuda"
SENT, ISENT = gi.SENT, gi.ISENT
RATIOS = {}
pkg, ibits, off4 = gi.pkg, gi.ibits, gi.off4


def i32(x, shift=False):
    t = torch.tensor(list(x), dtype=torch.int32)
    return off4(t) if shift else t.to(DEV)


def run_logits(q, w, pool, bt, lens, ld, shift=False, entry=None):
    """logits [B,T,ld] on the CPU, every entry pre-filled with SENT, inside guard bands that must keep SENT. shift: block_table, seqlens,
    weights and logits at 4 bytes past a 16-byte boundary. entry: the package function (the fp8 entry unless given)."""
    B, T = q.shape[:2]
    place = off4 if shift else (lambda t: t.to(DEV))
    big = torch.full(((B + 2) * T * ld + 8,), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
    o = 1 if shift else 0
    lg = big[T * ld + o:T * ld + o + B * T * ld].view(B, T, ld)
    assert not shift or lg.data_ptr() % 16 == 4
    (entry or pkg().mla_index_logits_paged_bf16_fp8)(q.to(DEV), place(w), pool.to(DEV), place(bt), place(torch.tensor(lens, dtype=torch.int32)), lg)
    torch.cuda.synchronize()
    flat = ibits(big).cpu()
    assert bool((flat[:T * ld + o] == SENT).all()) and bool((flat[T * ld + o + B * T * ld:] == SENT).all()), "guard bands of logits"
    return lg.cpu()


def check_logits(got, ref, bound, vis, label):
    worst = gi.check_logits(got, ref, bound, vis, label)  # asserts the sentinel at or past vis, finiteness and err <= bound; prints the ratio
    RATIOS[label.split(":")[0]] = max(RATIOS.get(label.split(":")[0], 0.0), worst)
    return worst


def run_append(p, pow2, shift=False, start=None, twice=None):
    """The pool after the append on the device, inside a guard page on each side; every byte starts as x8.MARK_BYTE (or as `start`).
    Returns (pool on the CPU, the two guard pages). twice: a second problem dict appended behind the first."""
    page, P = p["page"], p["P"]
    whole = torch.full((P + 2, page, x8.ROW), x8.MARK_BYTE, dtype=U8, device=DEV)
    pd = whole[1:P + 1]
    if start is not None:
        pd.copy_(start)
    assert pd.is_contiguous() and pd.data_ptr() % 16 == 0
    for prob in (p,) + ((twice,) if twice else ()):
        pkg().kv_append_paged_index_bf16_fp8(prob["k_new"].to(DEV), pd, i32(prob["bt"].flatten(), shift).view(prob["bt"].shape), i32(prob["lens"], shift),
                                             i32(prob["cu"], shift), pow2)
    torch.cuda.synchronize()
    out = whole.cpu()
    return out[1:P + 1], out[[0, P + 1]]


# ---------------------------------------------------------------------------------------------------- 1. the append

@pytest.mark.parametrize("pow2", [False, True], ids=["plain", "pow2"])
@pytest.mark.parametrize("page", x8.APPEND_PAGES)
@pytest.mark.parametrize("name", ix.APPEND_CASES)
def test_append_edges_byte_for_byte(built, dev, name, page, pow2):
    """The twelve edges of the append's contract (mla_index_reference.append_problem's recipes) behind pages of 16, 64 and 256 slots, with
    and without the power-of-two scale: every pool byte, the guard pages included, equals the CPU reference -- the codes, the scales, and
    the marker in every byte that is not a live token's."""
    p = x8.append_problem(name, page)
    start = x8.marked_pool(p["P"], page)
    want = x8.append_ref(start, p["bt"], p["lens"], p["cu"], p["k_new"], pow2)
    got, guards = run_append(p, pow2)
    assert bool((guards == x8.MARK_BYTE).all()), "guard pages of the pool"
    assert torch.equal(got, want), (name, page, pow2, int((got != want).sum()))
    assert int((got != x8.MARK_BYTE).sum()) > 0


@pytest.mark.parametrize("pow2", [False, True], ids=["plain", "pow2"])
def test_append_zero_keys_signed_zeros_and_amax_of_both_signs(built, dev, pow2):
    """An all-zero key (scale 1e-4 / 448, codes 0), a key of +-0 only (the signs survive), keys whose amax is a negative and a positive
    element, a key whose amax / 448 is a power of two already, a key below the floor: byte for byte."""
    k = x8.special_rows()
    n = k.shape[0]
    p = dict(page=16, P=3, bt=torch.tensor([[2, 0]], dtype=torch.int32), lens=[n + 13], cu=[0, n], k_new=k)  # slots 13 ... 18: across a page edge
    want = x8.append_ref(x8.marked_pool(3, 16), p["bt"], p["lens"], p["cu"], k, pow2)
    got, guards = run_append(p, pow2)
    assert torch.equal(got, want) and bool((guards == x8.MARK_BYTE).all())
    codes, scales = x8.views(got)
    assert float(scales[2, 13]) == (2.0 ** -22 if pow2 else float(torch.tensor(1e-4) / torch.tensor(448.0))) and bool((codes.view(U8)[2, 13] == 0).all())
    assert set(codes.view(U8)[2, 14].tolist()) == {0x00, 0x80}


@pytest.mark.parametrize("name", ["ragged", "b37", "cu_outside"])
def test_append_with_int_operands_four_bytes_past_a_boundary(built, dev, name):
    p = x8.append_problem(name, 64)
    want = x8.append_ref(x8.marked_pool(p["P"], 64), p["bt"], p["lens"], p["cu"], p["k_new"], True)
    got, guards = run_append(p, True, shift=True)
    assert torch.equal(got, want) and bool((guards == x8.MARK_BYTE).all())


def test_two_appends_in_a_row(built, dev):
    """A prompt, then one more token per sequence into the same pool: the second call leaves the first call's bytes alone."""
    page, B, max_pages = 16, 3, 4
    g = torch.Generator().manual_seed(3)
    first, P = [17, 5, 32], B * max_pages + 2
    bt = torch.randperm(P, generator=g)[:B * max_pages].to(torch.int32).view(B, max_pages)
    k0 = (torch.randn(sum(first), ix.D, generator=g) * 3).to(BF)
    k1 = (torch.randn(B, ix.D, generator=g) * 0.1).to(BF)
    p0 = dict(page=page, P=P, bt=bt, lens=first, cu=[0, 17, 22, 54], k_new=k0)
    p1 = dict(page=page, P=P, bt=bt, lens=[n + 1 for n in first], cu=[0, 1, 2, 3], k_new=k1)
    want = x8.append_ref(x8.append_ref(x8.marked_pool(P, page), bt, p0["lens"], p0["cu"], k0, True), bt, p1["lens"], p1["cu"], k1, True)
    got, guards = run_append(p0, True, twice=p1)
    assert torch.equal(got, want) and bool((guards == x8.MARK_BYTE).all())
    assert int((x8.views(got)[1].view(torch.int32) != x8.views(x8.marked_pool(P, page))[1].view(torch.int32)).sum()) == sum(first) + B


# ---------------------------------------------------------------------------------------------------- 2. logits against the bound

@pytest.mark.parametrize("name", sorted(x8.PARITY))
def test_logits_within_the_bound(built, dev, name):
    """Lengths 1, 15, 16, 17, 0, 255, 256, 257, 100 (Nmax 512) and 1023, 1024, -3, 1025, 2100, 300 (Nmax 2304: three chunks, ragged waves and
    blocks), Hi 1, 16, 17, 33, 64, T 1 and 3, pages 16, 64 and 256, ld below, equal to and above the cache and with ld % 4 = 1, 2, 3; keys of
    per-token magnitudes over 2^-4 ... 2^4 quantised with and without the power-of-two scale. Every j >= vis keeps the sentinel, the guard
    bands too; unlisted slots hold 0x7F codes and NaN scales."""
    q, w, (pool, bt), lens, ld = x8.parity_case(name)
    ref, bound, vis = x8.reference(name)
    got = run_logits(q, w, pool, bt, lens, ld)
    check_logits(got, ref, bound, vis, "logits %s: %s" % (name.split("-")[0], name))
    for b, n in enumerate(lens):
        if n <= 0:
            assert bool((ibits(got[b]) == SENT).all()), (name, b)


def test_logits_with_operands_four_bytes_past_a_boundary_and_a_second_call(built, dev):
    name = "small-Hi16-T3-p64"  # T ld = 1536 elements: the guard band in front keeps the logits at 4 bytes past a 16-byte boundary
    q, w, (pool, bt), lens, ld = x8.parity_case(name)
    base = run_logits(q, w, pool, bt, lens, ld)
    assert torch.equal(ibits(run_logits(q, w, pool, bt, lens, ld)), ibits(base))
    assert torch.equal(ibits(run_logits(q, w, pool, bt, lens, ld, shift=True)), ibits(base))


# ---------------------------------------------------------------------------------------------------- 3. exact answers

@pytest.mark.parametrize("page", [16, 256])
@pytest.mark.parametrize("Hi", [64, 33, 17])
def test_logits_exact_integers_and_power_of_two_scales(built, dev, Hi, page):
    """Integer q in [-4, 4], integer codes in [-8, 8], integer weights, scales 2^-3 ... 2^3: every partial sum is exact, so the result is the
    fp64 reference cast to fp32, bit for bit."""
    q, w, (pool, bt), lens, ld = x8.exact_case(Hi, 3, page)
    refs, _, vis = x8.logits_ref(q, w, pool, bt, lens, ld)
    got = run_logits(q, w, pool, bt, lens, ld)
    for b in range(len(lens)):
        for t in range(q.shape[1]):
            n = max(vis[b][t], 0)
            assert torch.equal(got[b, t, :n], refs["right"][b, t, :n].float()), (Hi, page, b, t)
            assert bool((ibits(got[b, t, n:]) == SENT).all())


@pytest.mark.parametrize("Hi", [64, 17])
def test_logits_with_unit_scales_equal_the_bf16_entry_on_the_same_codes(built, dev, Hi):
    q, w, (pool, bt), lens, ld = x8.exact_case(Hi, 3, 16, True)
    got = run_logits(q, w, pool, bt, lens, ld)
    other = run_logits(q, w, x8.bf16_pool(pool), bt, lens, ld, entry=pkg().mla_index_logits_paged_bf16)
    assert torch.equal(ibits(got), ibits(other))
    refs, _, vis = x8.logits_ref(q, w, pool, bt, lens, ld)
    fin = torch.isfinite(refs["right"])
    assert torch.equal(got[fin], refs["right"][fin].float()) and int(fin.sum()) > 1000


# ---------------------------------------------------------------------------------------------------- 4. order

@pytest.mark.parametrize("name", ["small-Hi33-T3-p16", "long-Hi64-T1-p64"])
def test_a_sequence_alone_gives_the_bits_it_gives_inside_the_batch(built, dev, name):
    q, w, (pool, bt), lens, ld = x8.parity_case(name)
    base = run_logits(q, w, pool, bt, lens, ld)
    for b in range(len(lens)):
        one = run_logits(q[b:b + 1].contiguous(), w[b:b + 1].contiguous(), pool, bt[b:b + 1].contiguous(), lens[b:b + 1], ld)
        assert torch.equal(ibits(one[0]), ibits(base[b])), (name, b)


# ---------------------------------------------------------------------------------------------------- 5. the chain

def test_chain_of_a_v32_step_on_e4m3_caches_eager_and_captured(built, dev):
    """Prompts of [2200, 130, 7, 0] tokens appended to an empty FP8 latent pool and an empty FP8 index pool; then one step: latent append
    -> fp8 index append -> fp8 logits -> top-k 64 -> fa2_decode_paged_mla_sparse_bf16_fp8, eagerly and replayed from one captured graph on
    fresh state. The index pool equals the CPU append reference byte for byte, the logits lie within the bound of the fp64 reference on that
    pool, the indices are the reference top-k of the GPU's own logits, O and LSE stay within the sparse entry's bound, and the graph gives the
    eager bits."""
    c = pkg()
    s8, mf, ml = t8.s8, t8.mf, t8.ml
    kvs, Hq, Hi, page, max_pages, B, topk = 0.003, 16, 64, 64, 36, 4, 64
    P = B * max_pages + 2
    g = torch.Generator().manual_seed(29)
    prompt = [2200, 130, 7, 0]
    new = [1, 1, 1, 0]  # the empty sequence appends nothing
    lens = [n + t for n, t in zip(prompt, new)]
    ld = max_pages * page
    table = c.kv_append_rope_table(ld, t8.DR).to(DEV)
    bt = torch.randperm(P, generator=g).to(torch.int32)[:B * max_pages].reshape(B, max_pages).contiguous()
    rnd = lambda *s: (torch.randn(*s, generator=g) * t8.SCALE).to(BF)  # noqa: E731
    keys = lambda n: (torch.randn(n, 128, generator=g) * 2.0 ** (torch.rand(n, 1, generator=g) * 8 - 4)).to(BF)  # noqa: E731
    n0, n1 = sum(prompt), sum(new)
    c0, k0, x0 = rnd(n0, t8.DC), rnd(n0, t8.DR), keys(n0)
    c1, k1, x1, q1 = rnd(n1, t8.DC), rnd(n1, t8.DR), keys(n1), ml.times(rnd(B, Hq, t8.DK), 128)
    qi, wt = torch.randn(B, 1, Hi, 128, generator=g).to(BF), torch.rand(B, 1, Hi, generator=g) * (Hi * 128) ** -0.5
    sc = mf.scale_t(kvs).to(DEV)
    cum = lambda xs: [sum(xs[:i]) for i in range(len(xs) + 1)]  # noqa: E731
    cu0, cu1 = t8.i32(cum(prompt)), t8.i32(cum(new))
    need = t8.plan(B, 1, Hq, topk, (torch.empty(P, page, t8.DK), bt))[2]

    def state():
        s = dict(pool=torch.full((P, page, t8.DK), t8.NAN_BYTE, dtype=U8, device=DEV).view(t8.F8), ipool=x8.empty_pool(P, page).to(DEV),
                 bt=bt.to(DEV), sl=t8.i32(prompt), qo=torch.full((B, Hq, t8.DK), t8.Q_FILL, dtype=torch.int16, device=DEV).view(BF),
                 logits=torch.full((B, 1, ld), SENT, dtype=torch.int32, device=DEV).view(torch.float32),
                 idx=torch.full((B, 1, topk), ISENT, dtype=torch.int32, device=DEV), ws=torch.empty(max(need, 16), dtype=U8, device=DEV))
        s["o"], s["lse"] = t8.outputs(B, 1, Hq)
        c.kv_append_paged_mla_bf16_fp8(c0.to(DEV), k0.to(DEV), s["pool"], s["bt"], s["sl"], cu0, sc, None, None, table, "interleaved")
        c.kv_append_paged_index_bf16_fp8(x0.to(DEV), s["ipool"], s["bt"], s["sl"], cu0, True)
        s["sl"].copy_(t8.i32(lens))
        torch.cuda.synchronize()
        return s

    fixed = tuple(t.to(DEV) for t in (c1, k1, x1, q1, qi, wt))

    def step(s):
        c.kv_append_paged_mla_bf16_fp8(fixed[0], fixed[1], s["pool"], s["bt"], s["sl"], cu1, sc, fixed[3][:n1], s["qo"][:n1], table, "interleaved")
        c.kv_append_paged_index_bf16_fp8(fixed[2], s["ipool"], s["bt"], s["sl"], cu1, True)
        c.mla_index_logits_paged_bf16_fp8(fixed[4], fixed[5], s["ipool"], s["bt"], s["sl"], s["logits"])
        c.mla_index_topk(s["logits"], s["sl"], topk, s["idx"])
        c.fa2_decode_paged_mla_sparse_bf16_fp8(s["qo"].view(B, 1, Hq, t8.DK), s["pool"], s["bt"], s["sl"], sc, s["idx"], t8.SCALE, s["o"], s["lse"], s["ws"])

    e = state()
    e["qo"][n1:].zero_()  # the empty sequence has no new token: its q row is not the append's to write
    step(e)
    torch.cuda.synchronize()
    pool, ipool, qo, lg, idx, o, lse = (e[k].cpu() for k in ("pool", "ipool", "qo", "logits", "idx", "o", "lse"))
    want = x8.append_ref(x8.append_ref(x8.empty_pool(P, page), bt, prompt, cum(prompt), x0, True), bt, lens, cum(new), x1, True)
    assert torch.equal(ipool, want)
    refs, bound, vis = x8.logits_ref(qi, wt, ipool, bt, lens, ld)
    check_logits(lg, refs["right"], bound, vis, "logits chain: Hi=64 T=1 page=64")
    clean = torch.where(ibits(lg) == SENT, torch.full_like(lg, ix.NAN), lg)
    assert torch.equal(idx, ix.topk_ref(clean, lens, topk))
    assert sorted(idx[2, 0].tolist()) == [-1] * (topk - lens[2]) + list(range(lens[2])) and idx[3, 0].tolist() == [-1] * topk
    assert len(set(idx[0, 0].tolist())) == topk and idx[0, 0].tolist() != list(range(topk))
    ref = s8.decode_sparse(qo.view(B, 1, Hq, t8.DK), pool, bt, lens, idx, kvs, t8.SCALE)
    RATIOS["chain O"] = t8.check(o, lse, *ref, "mla sparse fp8 on the fp8 indexer's list")
    gs = state()
    gs["qo"][n1:].zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(gs)
    torch.cuda.synchronize()
    assert bool((t8.bits(gs["o"].cpu()) == t8.O_FILL).all()) and bool((gs["idx"].cpu() == ISENT).all())  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gs["ipool"].cpu(), ipool) and torch.equal(ibits(gs["logits"].cpu()), ibits(lg)) and torch.equal(gs["idx"].cpu(), idx)
    assert torch.equal(t8.bits(gs["o"].cpu()), t8.bits(o)) and torch.equal(t8.fbits(gs["lse"].cpu()), t8.fbits(lse))


# ---------------------------------------------------------------------------------------------------- 6. summary

def test_zz_summary_of_error_over_bound(built, dev):
    """The largest err / bound of every group of this file. Not an assertion of its own -- every case asserted
    err <= bound where it ran."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
