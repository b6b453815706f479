"""Helpers of the attention-sink paged attention tests (tests/test_paged_sink_surface.py, tests/test_gpu_paged_sink_attention.py): the fp64
reference and the bf16 emulation of paged_window_reference with one sink logit per query head, the sink sets the tests use, and mirrors of the two
describe texts.

A sink is one fp32 logit per query head, in natural-log units and not scaled by 1/sqrt(D). For a row of head h that sees the keys lo <= j < n
(the window's mask, paged_window_reference), with s_j = q.k_j / sqrt(D):
    O = sum_j exp(s_j) v_j / (sum_j exp(s_j) + exp(sink_h)),  LSE = ln(sum_j exp(s_j) + exp(sink_h)).
A row that sees no key has O = 0 and LSE = -inf whatever the sink is. `count` counts the sink that many times (sink + ln count; 0: not at all):
the surface test uses 0 and 2 to show that the GPU cases would notice a dropped or a double-counted sink.

The criteria are those of the bf16 tests, no new tolerance: O is held to paged_bf16_reference.o_bound(emul, ref), LSE to decode_reference.lse_tol
(per head here, so that a head with a sink of 1e30 does not widen the tolerance of its neighbours), -inf rows and zero rows exactly. The emulation
is paged_window_reference.emul_rows -- scores in fp32, P = exp2 of the scores minus the row's FINAL maximum over the keys, P rounded to bf16, the
fp32 row sum of the unrounded P -- and then the sink as the kernels fold it, in fp32: sink2 = sink log2(e), m' = max(m, sink2), f = exp2(m - m'),
l' = l f + exp2(sink2 - m'), O scaled by f, divided by l' and rounded to bf16.

Largest err / bound of O seen on an MI355X over every case of tests/test_gpu_paged_sink_attention.py: prefill 0.319 (D = 64, G = 1, page 64,
W = 65, randn sinks), decode with one split 0.325 (D = 128, T = 3, G = 4, W = 33, mixed sinks), with several splits 0.372 (D = 128, T = 1, G = 1,
no window, len 4096), the gpt-oss layer shape 0.279, sinks of +30 0.314. No case exceeds 0.8. LSE: at most 0.0002 of lse_tol.

A plain module: nothing here is collected."""
import math

import torch

import multi_decode_reference as mr
import paged_decode_reference as pr
import paged_window_reference as wr
import prefill_reference as pf

LOG2E = wr.LOG2E
INT_MAX = wr.INT_MAX
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------------------- sink sets

def near(n_keys):
    """A sink the size of a typical row's log-sum-exp: n_keys scores of unit variance sum to about n_keys exp(1/2). Such a sink about halves O:
    counting it zero times or twice moves O by a third to a half of its size, far more than any bound."""
    return round(math.log(max(n_keys, 1)) + 0.5, 2)


def sinks_randn(Hq, seed=0):
    """randn * 2, fp32 [Hq]."""
    return torch.randn(Hq, generator=torch.Generator().manual_seed(7919 + seed)) * 2.0


def sinks_const(Hq, value):
    return torch.full((Hq,), value, dtype=torch.float32)


def sinks_mixed(Hq, n_keys):
    """[near, -inf, +1e30, 0, -1e30, +30, near + 1, near - 1] cycled over the heads: the first head always has the sensitive one."""
    c = near(n_keys)
    base = [c, NEG_INF, 1e30, 0.0, -1e30, 30.0, c + 1.0, c - 1.0]
    return torch.tensor([base[h % len(base)] for h in range(Hq)], dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------- describe texts

SINK_CLAUSE = ("the sink of a row's head (fp32, natural log, unscaled) is folded into the fp32 (m, l) of the finished row %s, once, and a row that "
               "sees no key stays O = 0, LSE = -inf")


def describe_prefill_text(B, total_q, Hq, Hkv, max_pages, page, D, W):
    """The text of cln_fa2_prefill_paged_varlen_window_sink_bf16_describe: the window text with the kernel's name and the sink clause."""
    text = wr.describe_prefill_text(B, total_q, Hq, Hkv, max_pages, page, D, W)
    assert text.count("fa2_prefill_paged_varlen_window_bf16_mfma<") == 1 and text.endswith("; deterministic")
    text = text.replace("fa2_prefill_paged_varlen_window_bf16_mfma<", "fa2_prefill_paged_varlen_window_sink_bf16_mfma<")
    return text[:-len("deterministic")] + SINK_CLAUSE % "in the epilogue" + "; deterministic"


def describe_multi_text(B, T, Hq, Hkv, max_pages, page, D, W):
    """The text of cln_fa2_decode_paged_multi_window_sink_bf16_describe: the window text with the kernels' names and where the sink is folded."""
    text = wr.describe_multi_text(B, T, Hq, Hkv, max_pages, page, D, W)
    assert text.count("fa2_decode_paged_multi_window_bf16_mfma<") == 1 and text.endswith("; deterministic")
    text = text.replace("fa2_decode_paged_multi_window_bf16_mfma<", "fa2_decode_paged_multi_window_sink_bf16_mfma<")
    text = text[:-len("; deterministic")]
    if wr.plan(B, T, Hq, Hkv, max_pages, page, D, W)[0] == 1:
        return text + "; " + SINK_CLAUSE % "at its final store" + "; deterministic"
    assert text.count("fa2_decode_combine_window_bf16_rows<") == 1
    text = text.replace("fa2_decode_combine_window_bf16_rows<", "fa2_decode_combine_window_sink_bf16_rows<")
    return (text + " and folds the sink of the row's head (fp32, natural log, unscaled) into the merged fp32 (m, l), once: the splits store raw "
            "partials, and a row that sees no key stays O = 0, LSE = -inf; deterministic")


# ---------------------------------------------------------------------------------------------------- reference and emulation

def emul_rows(q, k, v, vis, lo, sink):
    """paged_window_reference.emul_rows with the sink (an fp32 scalar tensor) of the rows' head folded in as the kernels do it. O_emul fp64 [R,D]
    holding bf16 values."""
    R, D = q.shape
    out = torch.zeros(R, D, dtype=torch.float64)
    top = int(max(vis)) if len(vis) else 0
    if top == 0:
        return out
    vist, lot = torch.tensor(list(vis), dtype=torch.int64), torch.tensor(list(lo), dtype=torch.int64)
    live = vist > lot
    j = torch.arange(top)[None, :]
    s = (q.double() @ k[:top].double().T).float() * torch.tensor(LOG2E / D ** 0.5, dtype=torch.float32)
    s = s.masked_fill((j >= vist[:, None]) | (j < lot[:, None]), NEG_INF)[live]
    m = s.max(dim=-1, keepdim=True).values                                     # the row's final maximum over the keys
    p = torch.exp2(s - m)
    lsum = p.sum(dim=-1, dtype=torch.float32)
    o = p.bfloat16().double() @ v[:top].double()
    sink2 = sink.float() * torch.tensor(LOG2E, dtype=torch.float32)           # formed once, in fp32
    m = m[:, 0]
    mn = torch.maximum(m, sink2)
    f = torch.exp2(m - mn)
    lsum = lsum * f + torch.exp2(sink2 - mn)
    out[live] = ((o * f.double()[:, None]).float().double() / lsum.double()[:, None]).float().bfloat16().double()
    return out


def _sequence(qb, kd, vd, vis, W, sinks, count):
    """paged_window_reference._sequence with sinks fp32 [Hq]: (O fp64 [T,Hq,D], LSE fp64 [T,Hq], O_emul fp64 [T,Hq,D])."""
    T, Hq, D = qb.shape
    G = Hq // kd.shape[0]
    vis = [int(x) for x in vis]
    lo = [max(0, n - W) for n in vis]
    O = torch.zeros(T, Hq, D, dtype=torch.float64)
    L = torch.full((T, Hq), NEG_INF, dtype=torch.float64)
    E = torch.zeros(T, Hq, D, dtype=torch.float64)
    top = max(vis) if vis else 0
    if top == 0:
        return O, L, E
    vist, lot = torch.tensor(vis), torch.tensor(lo)
    live = vist > 0
    j = torch.arange(top)[None, :]
    hidden = ((j >= vist[:, None]) | (j < lot[:, None]))[live]  # [T', top]
    for h in range(Hq):
        kh, vh = kd[h // G, :top].double(), vd[h // G, :top].double()
        s = (qb[live, h].double() @ kh.T / D ** 0.5).masked_fill(hidden, NEG_INF)
        sink = sinks[h].double() + math.log(count) if count else torch.tensor(NEG_INF, dtype=torch.float64)
        lse = torch.logaddexp(torch.logsumexp(s, dim=-1), sink)  # no overflow for a sink of 1e30
        O[live, h] = torch.exp(s - lse[:, None]) @ vh
        L[live, h] = lse
        E[:, h] = emul_rows(qb[:, h], kd[h // G], vd[h // G], vis, lo, sinks[h])
    return O, L, E


def prefill(q, k_pages, v_pages, block_table, lens, cu, W, sinks, count=1):
    """(O [total_q,Hq,D], LSE [total_q,Hq], O_emul) of the packed q, all fp64; NaN in the rows of no sequence. W = None: no window."""
    W = INT_MAX if W is None else W
    Nmax = block_table.shape[1] * k_pages.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (k_pages, v_pages))
    O = torch.full(q.shape, float("nan"), dtype=torch.float64)
    L = torch.full(q.shape[:2], float("nan"), dtype=torch.float64)
    E = torch.full(q.shape, float("nan"), dtype=torch.float64)
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        if hi > lo:
            O[lo:hi], L[lo:hi], E[lo:hi] = _sequence(q[lo:hi], k[b], v[b], pf.visible([lens[b]], hi - lo, Nmax)[0].tolist(), W, sinks, count)
    return O, L, E


def decode(q, k_pages, v_pages, block_table, lens, W, sinks, count=1):
    """(O [B,T,Hq,D], LSE [B,T,Hq], O_emul), all fp64. W = None: no window."""
    W = INT_MAX if W is None else W
    B, T = q.shape[:2]
    Nmax = block_table.shape[1] * k_pages.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (k_pages, v_pages))
    vis = mr.visible(lens, T, Nmax)
    got = [_sequence(q[b], k[b], v[b], vis[b * T:(b + 1) * T], W, sinks, count) for b in range(B)]
    return tuple(torch.stack([g[i] for g in got]) for i in range(3))


# ---------------------------------------------------------------------------------------------------- the cases both test files look at
# Made on the CPU, once per process, never modified. The surface test shows without a GPU that the cases marked sensitive would notice a sink
# counted zero times or twice; the GPU test runs them.

import functools  # noqa: E402

BF = torch.bfloat16
PAGE = 16

# prefill: packed sequences of [17, 0, 3, 1, 4] new tokens behind contexts of 63 / 0 / 200 / 5 keys; the last has len_b = 2 < T_b = 4, so its first
# two tokens see no key. With G = 8 the 17 tokens are 136 rows: two row tiles.
PREFILL_T = [17, 0, 3, 1, 4]
PREFILL_LENS = [80, 0, 203, 6, 2]
PREFILL_NMAX = 256
PREFILL_HEADS = [(1, 1), (8, 1), (8, 2)]  # (Hq, Hkv)
PREFILL_PAGES = [16, 64]
PREFILL_WINDOWS = [1, 65, 128, INT_MAX]


@functools.lru_cache(maxsize=None)
def prefill_case(D, Hq, Hkv, page):
    """(qs per sequence, lens, (k_pages, v_pages, block_table))."""
    g = torch.Generator().manual_seed(17 * D + 3 * Hq + Hkv + page)
    qs = tuple(torch.randn(t, Hq, D, generator=g).to(BF) for t in PREFILL_T)
    k, v = (torch.randn(len(PREFILL_T), Hkv, PREFILL_NMAX, D, generator=g).to(BF) for _ in range(2))
    return qs, PREFILL_LENS, pr.make_pool(k, v, page, PREFILL_LENS, seed=page)


def prefill_sinks(Hq, W):
    """The sensitive set of a prefill case: `near` the log-sum-exp of the first sequence's rows, which see min(W, 64 … 80) keys."""
    return sinks_mixed(Hq, min(W, 64))


def pack(qs, first=0, spare=0):
    """(q [total_q,Hq,D], cu): the sequences packed from row `first` on; the rows of no sequence hold 2^100."""
    cu = [first]
    for x in qs:
        cu.append(cu[-1] + x.shape[0])
    q = torch.full((cu[-1] + spare,) + tuple(qs[0].shape[1:]), 2.0 ** 100, dtype=BF)
    for b, x in enumerate(qs):
        q[cu[b]:cu[b + 1]] = x
    return q, cu


# decode: T in {1, 3, 8} x G in {1, 4, 8} gives 1, 2, 3 and 4 row tiles of 16
DECODE_T, DECODE_G = [1, 3, 8], [1, 4, 8]
DECODE_LENS = [4096, 1024, 257, 100, 0]
ONE_HKV, ONE_NMAX, ONE_W = 8, 4096, 33         # one split: B = 5
SPLIT_NMAX, SPLIT_WINDOWS = 16384, [1000, None]  # several splits: B = 1, Hkv = 1, one call per length


@functools.lru_cache(maxsize=None)
def _dense(B, Hkv, Nmax, D):
    g = torch.Generator().manual_seed(B + 10 * Hkv + Nmax + D)
    return tuple(torch.randn(B, Hkv, Nmax, D, generator=g).to(BF) for _ in range(2))


@functools.lru_cache(maxsize=None)
def decode_one_case(T, G, D):
    """(q [5,T,Hq,D], lens, pool) of the one-split shape."""
    k, v = _dense(len(DECODE_LENS), ONE_HKV, ONE_NMAX, D)
    q = torch.randn(len(DECODE_LENS), T, ONE_HKV * G, D, generator=torch.Generator().manual_seed(100 * T + G + D)).to(BF)
    return q, DECODE_LENS, pr.make_pool(k, v, PAGE, DECODE_LENS, seed=T + G)


@functools.lru_cache(maxsize=None)
def decode_split_case(T, G, D, n):
    """(q [1,T,G,D], [n], pool) of the several-splits shape with one sequence of n keys."""
    k, v = _dense(1, 1, SPLIT_NMAX, D)
    q = torch.randn(1, T, G, D, generator=torch.Generator().manual_seed(1000 * T + G + D + n)).to(BF)
    return q, [n], pr.make_pool(k, v, PAGE, [n], seed=n % 89)


def decode_split_sinks(G, n, W):
    """The sensitive set of a several-splits case: `near` the log-sum-exp of a row that sees min(W, n) keys."""
    return sinks_mixed(G, n if W is None else min(W, n))
