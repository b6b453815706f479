"""Helpers of the multi-head latent attention prefill tests (tests/test_mla_prefill_surface.py, tests/test_gpu_mla_prefill.py):
the fp64 reference and the bf16 emulation of cuda_learn_notes_amd.fa2_prefill_varlen_mla_bf16, the fp64 merge of two attention states, and the
cases of the GPU test.

Per head h the key of token j is [k_nope_h (128) | k_pe (64)] -- k_pe one row per token, shared by every head -- and the value v_h (128); kv is
[total_k, Hq, 256] = [k_nope | v]. Sequence b has T_b queries (cu_q) and L_b keys (cu_k); query t sees the keys j < n = L_b - (T_b - 1 - t)
(causal) or all L_b:
    s_j = scale q . key_j,   O = softmax(s) V,   LSE = ln sum_j exp(s_j);   no key: O = 0, LSE = -inf.
With v = k_nope and one head this IS paged_mla_reference.decode(..., dv=128) on latent rows [k_nope | k_pe] of dk = 192, which the surface test
asserts -- the reference is not free-standing.

The emulation follows paged_bf16_reference.emul_rows' six steps with the caller's scale, a 192-dim key and a 128-dim value (the code of
paged_mla_reference.emul_rows with the value a tensor of its own). The criteria are the family's, no new tolerance for the attention: O within
paged_bf16_reference.o_bound(emul, ref), LSE within decode_reference.lse_tol, -inf rows and zero rows exactly.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools
import math

import torch

import paged_softcap_reference as cr

BF = torch.bfloat16
DN, DR, DQ, DV, DKV = 128, 64, 192, 128, 256
MAX_HQ = 128
LOG2E = cr.LOG2E
NEG_INF = float("-inf")
SCALE = 192 ** -0.5
YARN = SCALE * (0.1 * math.log(40) + 1) ** 2  # DeepSeek-V3 / R1 with YaRN (mscale^2 at factor 40): about 0.1353
QUARTER = SCALE / 4
OTHER_SCALES = (YARN, QUARTER)  # scales that are not the test data's
Q_MULT = 1  # q and the keys are standard normal: the scores have standard deviation 1 at SCALE and the softmax is far from flat as it is


# ---------------------------------------------------------------------------------------------------- reference and emulation

def visible(T, L, causal):
    """The keys query t = 0 .. T - 1 of a sequence with L keys sees."""
    return [max(L - (T - 1 - t), 0) if causal else max(L, 0) for t in range(T)]


def emul_rows(q, k, v, vis, scale):
    """O_emul fp64 [R, dv] holding bf16 values: queries q [R, dk] over keys k [N, dk] and values v [N, dv] (bf16), query r seeing the first
    vis[r] keys."""
    R = q.shape[0]
    out = torch.zeros(R, v.shape[1], dtype=torch.float64)
    top = int(max(vis)) if len(vis) else 0
    if top == 0:
        return out
    vist = torch.tensor(list(vis), dtype=torch.int64)
    live = vist > 0
    s = (q.double() @ k[:top].double().T).float() * torch.tensor(cr.f32(scale) * LOG2E, dtype=torch.float32)   # 1
    s = s.masked_fill(torch.arange(top)[None, :] >= vist[:, None], NEG_INF)[live]
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)                                                   # 2
    lsum = p.sum(dim=-1, dtype=torch.float32)                                                                 # 5: of the unrounded P
    o = p.bfloat16().double() @ v[:top].double()                                                              # 3, 4
    out[live] = (o / lsum.double()[:, None]).float().bfloat16().double()                                      # 5, 6
    return out


def offsets(cu, total):
    """(first row, count) per sequence from offsets clamped as the kernel clamps them."""
    c = [min(max(int(x), 0), total) for x in cu]
    return [(c[b], max(c[b + 1] - c[b], 0)) for b in range(len(c) - 1)]


def prefill(q, kv, k_pe, cu_q, cu_k, scale, causal=True):
    """(O [total_q,Hq,128], LSE [total_q,Hq], O_emul [total_q,Hq,128]), all fp64, NaN in the rows of no sequence: q bf16 [total_q,Hq,192], kv
    bf16 [total_k,Hq,256], k_pe bf16 [total_k,64]."""
    total_q, Hq, _ = q.shape
    x = cr.f32(scale)
    O = torch.full((total_q, Hq, DV), float("nan"), dtype=torch.float64)
    L = torch.full((total_q, Hq), float("nan"), dtype=torch.float64)
    E = torch.full((total_q, Hq, DV), float("nan"), dtype=torch.float64)
    for (q0, T), (k0, n) in zip(offsets(cu_q, total_q), offsets(cu_k, kv.shape[0])):
        if T == 0:
            continue
        vis = visible(T, n, causal)
        rows = slice(q0, q0 + T)
        O[rows], L[rows], E[rows] = 0.0, NEG_INF, 0.0
        top = max(vis)
        if top == 0:
            continue
        vist = torch.tensor(vis)
        live = vist > 0
        hidden = (torch.arange(top)[None, :] >= vist[:, None])[live]
        for h in range(Hq):
            key = torch.cat([kv[k0:k0 + top, h, :DN], k_pe[k0:k0 + top]], dim=-1)
            val = kv[k0:k0 + top, h, DN:]
            s = (q[rows, h][live].double() @ key.double().T * x).masked_fill(hidden, NEG_INF)
            lse = torch.logsumexp(s, dim=-1)
            o_h, l_h = O[rows, h], L[rows, h]
            o_h[live] = torch.exp(s - lse[:, None]) @ val.double()
            l_h[live] = lse
            O[rows, h], L[rows, h] = o_h, l_h
            E[rows, h] = emul_rows(q[rows, h], key, val, vis, scale)
    return O, L, E


def merge(o_a, lse_a, o_b, lse_b):
    """The fp64 merge of two attention states: (O [..., D], LSE [...]). A side whose LSE is -inf is selected out, whatever its O holds."""
    oa, ob, la, lb = o_a.double(), o_b.double(), lse_a.double(), lse_b.double()
    m = torch.maximum(la, lb)
    ms = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    wa, wb = torch.exp(la - ms), torch.exp(lb - ms)   # exp(-inf) = 0
    oa = torch.where((la == NEG_INF)[..., None], torch.zeros_like(oa), oa)
    ob = torch.where((lb == NEG_INF)[..., None], torch.zeros_like(ob), ob)
    ws = wa + wb
    dead = ws == 0
    o = (wa[..., None] * oa + wb[..., None] * ob) / torch.where(dead, torch.ones_like(ws), ws)[..., None]
    o = torch.where(dead[..., None], torch.zeros_like(o), o)
    return o, torch.where(dead, torch.full_like(m, NEG_INF), ms + torch.log(ws))


def merge_bound(ref, o_a, o_b):
    """Per element 2^-8 |r| + 2^-20 max(|O_a|, |O_b|): one rounding to bf16 (the append's first term), and the fp32 evaluation of two
    exponentials, a sum, a quotient and two products at 2^-23 each under a factor of 8."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -20 * torch.maximum(o_a.double().abs(), o_b.double().abs())


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test

# (T, context = L - T, Hq): every T of 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257, every context of 0, 1, 63, 64, 65 and both head counts
ONE_CASES = [(1, 0, 1), (15, 1, 3), (16, 63, 1), (17, 64, 3), (31, 65, 1), (32, 0, 3), (33, 1, 1), (127, 63, 3), (128, 64, 1), (129, 65, 3),
             (257, 0, 1), (257, 65, 3), (1, 64, 3), (128, 1, 3)]
RAGGED_T = [129, 0, 1, 64, 33]
RAGGED_L = [129, 5, 65, 64, 233]      # T + [0, 5, 64, 0, 200]
SHORT_T, SHORT_L = [40, 17], [25, 17]  # a sequence with L_b < T_b: its first 15 rows see no key
FRONT, BACK = 3, 5                     # cu_q[0] = 3, trailing rows past cu_q[B]
COUNT_N = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129]
MERGE_D, MERGE_ROWS = [8, 128, 512], [1, 257]
CHAIN_C, CHAIN_T = [64, 100], 33


def cu_of(counts, front=0):
    cu = [front]
    for c in counts:
        cu.append(cu[-1] + c)
    return cu


def _randn(shape, g):
    return torch.randn(*shape, generator=g).to(BF)


@functools.lru_cache(maxsize=None)
def packed_case(Ts, Ls, Hq, seed=0, front=0, back=0):
    """(q [front + sum T + back, Hq, 192], kv [front + sum L + back, Hq, 256], k_pe [.., 64], cu_q, cu_k) of standard normal values."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * sum(Ts) + sum(Ls) + Hq)
    cu_q, cu_k = cu_of(Ts, front), cu_of(Ls, front)
    tq, tk = cu_q[-1] + back, cu_k[-1] + back
    return _randn((tq, Hq, DQ), g), _randn((tk, Hq, DKV), g), _randn((tk, DR), g), cu_q, cu_k


def one_case(T, ctx, Hq):
    return packed_case((T,), (T + ctx,), Hq)


@functools.lru_cache(maxsize=None)
def scale_case(causal, scale, Hq=3):
    """(q, kv, k_pe, cu_q, cu_k, the reference at scale, the reference at SCALE) of the ragged packed batch of the GPU test."""
    Ts, Ls = tuple(RAGGED_T + SHORT_T), tuple(RAGGED_L + SHORT_L)
    q, kv, k_pe, cu_q, cu_k = packed_case(Ts, Ls, Hq, seed=1, front=FRONT, back=BACK)
    return q, kv, k_pe, cu_q, cu_k, prefill(q, kv, k_pe, cu_q, cu_k, scale, causal), prefill(q, kv, k_pe, cu_q, cu_k, SCALE, causal)
