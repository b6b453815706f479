"""Helpers of the tests of the paged bf16 attention entries with a softmax scale and logit soft-capping (tests/test_paged_softcap_surface.py,
tests/test_gpu_paged_softcap_attention.py): the fp64 reference and the bf16 emulation of paged_sink_reference /
paged_bf16_fp8_reference with `scale` and `cap`, six defects that can be switched on, and the cases both test files look at.

With x = the softmax scale in use (scale, or 1 / sqrt(D) for None), a row of head h that sees the keys lo <= j < n has u_j = q.k_j x and
    s_j = u_j (cap None)  or  cap tanh(u_j / cap),
    O = sum_j exp(s_j) v_j / (sum_j exp(s_j) + exp(sink_h)),  LSE = ln(sum_j exp(s_j) + exp(sink_h)).
The sink is neither scaled nor capped; the mask comes after the cap (a hidden key is -inf, not -cap); a row that sees no key has O = 0 and
LSE = -inf. Over FP8 pools the reference runs on the dequantised float64 pools (paged_bf16_fp8_reference.dq, exact), so k_scale is part of u_j
and stands inside the tanh. scale and cap are taken as the fp32 numbers the C entries receive.

The criteria are the families', no new tolerance: O within paged_bf16_reference.o_bound(emul, ref), LSE within decode_reference.lse_tol per head,
-inf rows and zero rows exactly (test_gpu_paged_sink_attention.check). The emulation, in order: the score is the fp32 value of q.k; with a cap it
is multiplied by pre = x / cap in fp32, goes through torch.tanh in fp32 and is multiplied by cap2 = cap log2(e) in fp32; without a cap it is
multiplied by the fp32 multiplier x log2(e); then paged_sink_reference.emul_rows as it stands -- P = exp2 of the score minus the row's final
maximum, P rounded to bf16, the fp32 row sum of the unrounded P, the sink folded in fp32.

The defects, for the fp64 reference only (the surface test shows that each moves O past the bound on the cases that exist for it):
    "nocap"           the cap is ignored;
    "cap_after_mask"  the mask comes first: hidden keys become -cap;
    "cap_sink"        the sink is capped too;
    "default_scale"   1 / sqrt(D) is used instead of the given scale;
    "scale_outside"   x cap tanh(q.k / cap);
    "no_kscale"       FP8 only: k_scale left out of the tanh argument, cap tanh(u / k_scale / cap).

Largest err / bound of O seen on an MI355X: see DESIGN 4.4.14 and profiles/r25_paged_softcap_tests.log.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools
import math

import torch

import multi_decode_reference as mr
import paged_anyg_cases as ac
import paged_bf16_fp8_reference as fr
import paged_decode_reference as pr
import paged_sink_reference as sr
import prefill_reference as pf

BF = torch.bfloat16
LOG2E = sr.LOG2E
INT_MAX = sr.INT_MAX
NEG_INF = float("-inf")
DEFECTS = ("nocap", "cap_after_mask", "cap_sink", "default_scale", "scale_outside", "no_kscale")


def f32(x):
    """The fp32 number a C entry receives for the Python float x, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def scale_in_use(scale, D):
    return 1.0 / math.sqrt(D) if scale is None else f32(scale)


# ---------------------------------------------------------------------------------------------------- reference and emulation

def emul_rows(q, k, v, vis, lo, sink, scale, cap):
    """paged_sink_reference.emul_rows with the softmax scale and the cap: only the line that forms the scores differs. O_emul fp64 [R,D] holding
    bf16 values."""
    R, D = q.shape
    out = torch.zeros(R, D, dtype=torch.float64)
    top = int(max(vis)) if len(vis) else 0
    if top == 0:
        return out
    vist, lot = torch.tensor(list(vis), dtype=torch.int64), torch.tensor(list(lo), dtype=torch.int64)
    live = vist > lot
    j = torch.arange(top)[None, :]
    x = scale_in_use(scale, D)
    s = (q.double() @ k[:top].double().T).float()
    if cap is None:
        s = s * torch.tensor(LOG2E / D ** 0.5 if scale is None else x * LOG2E, dtype=torch.float32)
    else:
        c = f32(cap)
        s = torch.tanh(s * torch.tensor(x / c, dtype=torch.float32)) * torch.tensor(c * LOG2E, dtype=torch.float32)
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


def scores64(raw, D, scale, cap, defect=None, k_scale=1.0):
    """s fp64 of the raw fp64 products q.k (over dequantised K), before the mask."""
    x = 1.0 / math.sqrt(D) if defect == "default_scale" else scale_in_use(scale, D)
    if cap is None or defect == "nocap":
        return raw * x
    c = f32(cap)
    if defect == "scale_outside":
        return x * c * torch.tanh(raw / c)
    if defect == "no_kscale":
        return c * torch.tanh(raw * x / float(k_scale) / c)
    return c * torch.tanh(raw * x / c)


def _sequence(qb, kd, vd, vis, W, sinks, scale, cap, defect, k_scale):
    """paged_sink_reference._sequence with scale, cap and a defect: (O fp64 [T,Hq,D], LSE fp64 [T,Hq], O_emul fp64 [T,Hq,D])."""
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
        s = scores64(qb[live, h].double() @ kh.T, D, scale, cap, defect, 1.0 if k_scale is None else k_scale[h // G])
        hide = -f32(cap) if defect == "cap_after_mask" and cap is not None else NEG_INF
        s = s.masked_fill(hidden, hide)
        sink = sinks[h].double()
        if defect == "cap_sink" and cap is not None:
            sink = f32(cap) * torch.tanh(sink / f32(cap))
        lse = torch.logaddexp(torch.logsumexp(s, dim=-1), sink)  # no overflow for a sink of 1e30
        O[live, h] = torch.exp(s - lse[:, None]) @ vh
        L[live, h] = lse
        if defect is None:
            E[:, h] = emul_rows(qb[:, h], kd[h // G], vd[h // G], vis, lo, sinks[h], scale, cap)
    return O, L, E


def _pools(k_pages, v_pages, ks, vs):
    return (k_pages, v_pages) if ks is None else (fr.dq(k_pages, ks), fr.dq(v_pages, vs))


def _sinks(sinks, Hq):
    return torch.full((Hq,), NEG_INF, dtype=torch.float32) if sinks is None else sinks


def prefill(q, k_pages, v_pages, block_table, lens, cu, W, sinks, scale=None, cap=None, defect=None, ks=None, vs=None):
    """(O [total_q,Hq,D], LSE [total_q,Hq], O_emul) of the packed q, all fp64; NaN in the rows of no sequence. W = None: no window; sinks = None:
    no sink; ks, vs: the fp32 [Hkv] scales of e4m3 pools. With a defect O_emul stays 0."""
    W = INT_MAX if W is None else W
    kp, vp = _pools(k_pages, v_pages, ks, vs)
    Nmax = block_table.shape[1] * kp.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (kp, vp))
    sinks = _sinks(sinks, q.shape[1])
    O = torch.full(q.shape, float("nan"), dtype=torch.float64)
    L = torch.full(q.shape[:2], float("nan"), dtype=torch.float64)
    E = torch.full(q.shape, float("nan"), dtype=torch.float64)
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        if hi > lo:
            O[lo:hi], L[lo:hi], E[lo:hi] = _sequence(q[lo:hi], k[b], v[b], pf.visible([lens[b]], hi - lo, Nmax)[0].tolist(), W, sinks, scale, cap,
                                                     defect, ks)
    return O, L, E


def decode(q, k_pages, v_pages, block_table, lens, W, sinks, scale=None, cap=None, defect=None, ks=None, vs=None):
    """(O [B,T,Hq,D], LSE [B,T,Hq], O_emul), all fp64."""
    W = INT_MAX if W is None else W
    B, T = q.shape[:2]
    kp, vp = _pools(k_pages, v_pages, ks, vs)
    Nmax = block_table.shape[1] * kp.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (kp, vp))
    sinks = _sinks(sinks, q.shape[2])
    vis = mr.visible(lens, T, Nmax)
    got = [_sequence(q[b], k[b], v[b], vis[b * T:(b + 1) * T], W, sinks, scale, cap, defect, ks) for b in range(B)]
    return tuple(torch.stack([g[i] for g in got]) for i in range(3))


def dense(q, k, v, n, lo, sink, x, cap):
    """One row in fp64, written out: q [D], k, v [N,D], the keys lo <= j < n, the sink logit; (O [D], LSE). What the surface test holds the
    reference against."""
    if n <= lo:
        return torch.zeros(q.shape[0], dtype=torch.float64), NEG_INF
    if sink > 700.0:  # exp overflows fp64: the sink is all there is
        return torch.zeros(q.shape[0], dtype=torch.float64), sink
    num, den = torch.zeros(q.shape[0], dtype=torch.float64), math.exp(sink)
    for j in range(lo, n):
        u = float(q.double() @ k[j].double()) * x
        e = math.exp(u if cap is None else cap * math.tanh(u / cap))
        num, den = num + e * v[j].double(), den + e
    return num / den, math.log(den)


# ---------------------------------------------------------------------------------------------------- the cases both test files look at
# The shapes are tests/paged_anyg_cases.py's. randn scores have unit variance and a cap of 30 or 50 does nothing to them, so the sensitive cases
# multiply q by a power of two (exact in bf16) and take a small cap: with q x 4 the scores u have a standard deviation of about 4 (3.5 with the
# scale below), and with a cap of 2 most of them sit past the cap. The mixed sinks of paged_anyg_cases.sinks_for include +30, far above the cap.

Q_MUL, CAP = 4.0, 2.0
P1_G, P1_PAGES, P1_WINDOWS = [3, 8], ac.P1_PAGES, ac.P1_WINDOWS
P2_G = 3
D3_TG = [(1, 3), (8, 8), (4, 16)]
D4_TG, D4_LENS, D4_WINDOWS = (3, 5), ac.D4_LENS, ac.D4_WINDOWS
S5_G = [3, 8]  # the any-G entries' bits


def scale_for(D):
    """The sensitive scale: 1 / sqrt(1.3 D), neither the default nor a power of two."""
    return 1.0 / math.sqrt(1.3 * D)


def configs(D):
    """(name, scale, cap): the cap and the scale each on and off."""
    return [("plain", None, None), ("scale", scale_for(D), None), ("cap", None, CAP), ("scale+cap", scale_for(D), CAP)]


MODELS = {  # the three models' real numbers, on randn data: plain parity cases. (G, scale, cap, W); D = 128
    "gemma-2-27b": (2, 144 ** -0.5, 50.0, None),
    "gemma-3-27b": (2, 168 ** -0.5, None, 33),
    "grok-1": (6, None, 30.0, None),
}


@functools.lru_cache(maxsize=None)
def prefill_case(D, G, page):
    q, cu, lens, pool = ac.prefill_case(D, G, page)
    return (q.float() * Q_MUL).to(BF), cu, lens, pool


@functools.lru_cache(maxsize=None)
def ragged_case(D, G):
    qs, lens, pool = ac.ragged_case(D, G)
    return tuple((x.float() * Q_MUL).to(BF) for x in qs), lens, pool


@functools.lru_cache(maxsize=None)
def decode_one_case(T, G, D):
    q, lens, pool = ac.decode_one_case(T, G, D)
    return (q.float() * Q_MUL).to(BF), lens, pool


@functools.lru_cache(maxsize=None)
def decode_split_case(T, G, D, n):
    q, lens, pool = ac.decode_split_case(T, G, D, n)
    return (q.float() * Q_MUL).to(BF), lens, pool
