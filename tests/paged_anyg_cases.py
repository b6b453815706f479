"""The cases of the any-group-size paged attention tests (tests/test_paged_anyg_surface.py, tests/test_gpu_paged_anyg_attention.py; DESIGN
4.4.13): the *_anyg_* entries take every G = Hq / Hkv in 1 ... 16. The references are the families' own -- paged_sink_reference for bf16 pools,
paged_bf16_fp8_reference for e4m3 pools; both index the KV head as h // G -- and so are the criteria: O within
paged_bf16_reference.o_bound(emul, ref) = 2 max|O_emul - O_64| + 2^-8 max|O_64|, LSE within decode_reference.lse_tol per head, -inf rows and zero
rows exactly. No new tolerance.

What is new here is `mapped`: an fp64 model of HOW the kernels walk a (sequence, KV head) -- row r of its T G rows is (t, g) = (r / G, r mod G),
the row reads q and writes o at flat row c0 Hq + kvh G + t Hq + g, sees len - (T - 1 - t) keys and takes the sink of head kvh G + g; the packed
prefill gives sequence b the slots from cu_q[b] G / 128 + b of total_q G / 128 + B -- with three defects that can be switched on:
    "shift"  t = r >> ceil(log2 G), g = r & (2^ceil(log2 G) - 1): the power-of-two map on a G that is none;
    "sink8"  the sink of head kvh 8 + g;
    "slot"   the slots of a sequence from cu_q[b] Gpow2 / 128 + b, Gpow2 = 2^ceil(log2 G), in a grid sized with G.
The surface test shows on the CPU that the right map IS the reference and that each defect moves O past the bound on the cases that exist for
it; rows a defect never writes keep 0.

Largest err / bound of O seen on an MI355X: see DESIGN 4.4.13 and profiles/r24_paged_anyg_tests.log.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools

import torch

import paged_bf16_fp8_reference as fr
import paged_decode_reference as pr
import paged_sink_reference as sr

BF = torch.bfloat16
INT_MAX = sr.INT_MAX
NEG_INF = float("-inf")
ROW_TILE = 128

GROUPS = [3, 5, 6, 7, 12, 16]          # what the siblings refuse
POW2 = [1, 2, 4, 8]                    # what they take: the bits must agree

# 1. prefill, rows that straddle tiles: one sequence of 45 tokens behind 19 keys, Hkv = 2: 135 ... 720 rows
P1_T, P1_CTX, P1_HKV, P1_NMAX = 45, 19, 2, 128
P1_WINDOWS, P1_PAGES = [None, 33], [16, 64]
# 2. packed ragged prefill: 43 tokens x G = 3 are 129 rows, a full tile and one row
P2_T, P2_CTX, P2_HKV, P2_NMAX, P2_G, P2_W = [43, 0, 1, 26, 5], [0, 7, 200, 64, 3], 3, 256, [3, 7], 33
# 3. decode, one split: 1, 2, 3 and 4 row tiles and the edge T G = 64
D3_TG = [(1, 3), (3, 5), (4, 5), (8, 6), (8, 7), (5, 12), (1, 16), (4, 16)]
D3_HKV, D3_LENS, D3_NMAX, D3_WINDOWS, PAGE = 2, [0, 1, 17, 100, 257], 272, [None, 33], 16
# 4. decode, several splits: B = 1, Hkv = 1, max_pages page = 4096
D4_TG, D4_LENS, D4_NMAX, D4_WINDOWS = [(3, 5), (4, 16)], [4096, 1000], 4096, [None, 1000]
# 5. the siblings' bits
S5_PREFILL_G, S5_DECODE_TG = [4, 8], [(3, 4), (8, 8)]


def sinks_for(Hq, n_keys):
    """The family's mixed sinks (paged_sink_reference.sinks_mixed: near, -inf, +1e30, 0, -1e30, +30, near + 1, near - 1), moved on by one place
    every 8 heads: sinks_mixed has period 8, and with it head 8 + g would hold what head 16 + g holds -- the wrong sink head h 8 + g of a
    G = 16 case would go unseen."""
    m = sr.sinks_mixed(8, n_keys)
    return m[[(h + h // 8) % 8 for h in range(Hq)]].contiguous()


@functools.lru_cache(maxsize=None)
def prefill_case(D, G, page, T=P1_T, ctx=P1_CTX):
    """case 1: (q [T,Hq,D], cu, lens, pool)"""
    Hq = P1_HKV * G
    g = torch.Generator().manual_seed(31 * D + 7 * G + page + T)
    q = torch.randn(T, Hq, D, generator=g).to(BF)
    k, v = (torch.randn(1, P1_HKV, P1_NMAX, D, generator=g).to(BF) for _ in range(2))
    lens = [ctx + T]
    return q, [0, T], lens, pr.make_pool(k, v, page, lens, seed=G)


@functools.lru_cache(maxsize=None)
def ragged_case(D, G):
    """case 2: (qs per sequence, lens, pool)"""
    Hq = P2_HKV * G
    g = torch.Generator().manual_seed(13 * D + G)
    qs = tuple(torch.randn(t, Hq, D, generator=g).to(BF) for t in P2_T)
    k, v = (torch.randn(len(P2_T), P2_HKV, P2_NMAX, D, generator=g).to(BF) for _ in range(2))
    lens = [c + t for c, t in zip(P2_CTX, P2_T)]
    return qs, lens, pr.make_pool(k, v, PAGE, lens, seed=G)


@functools.lru_cache(maxsize=None)
def _dense(B, Hkv, Nmax, D):
    g = torch.Generator().manual_seed(3 * B + 10 * Hkv + Nmax + D)
    return tuple(torch.randn(B, Hkv, Nmax, D, generator=g).to(BF) for _ in range(2))


@functools.lru_cache(maxsize=None)
def decode_one_case(T, G, D):
    """case 3: (q [5,T,Hq,D], lens, pool)"""
    k, v = _dense(len(D3_LENS), D3_HKV, D3_NMAX, D)
    q = torch.randn(len(D3_LENS), T, D3_HKV * G, D, generator=torch.Generator().manual_seed(100 * T + G + D)).to(BF)
    return q, D3_LENS, pr.make_pool(k, v, PAGE, D3_LENS, seed=T + G)


@functools.lru_cache(maxsize=None)
def decode_split_case(T, G, D, n):
    """case 4: (q [1,T,G,D], [n], pool)"""
    k, v = _dense(1, 1, D4_NMAX, D)
    q = torch.randn(1, T, G, D, generator=torch.Generator().manual_seed(1000 * T + G + D + n)).to(BF)
    return q, [n], pr.make_pool(k, v, PAGE, [n], seed=n % 89)


def to_fp8(pool, Hkv):
    """(e4m3 pool, k_scale, v_scale) of a bf16 pool, with the per-head scales of paged_bf16_fp8_reference."""
    ks, vs = fr.scales(Hkv)
    return fr.quantize_pools(pool, ks, vs), ks, vs


# ---------------------------------------------------------------------------------------------------- the map, in fp64

def _pow2(G):
    c = 0
    while (1 << c) < G:
        c += 1
    return c


def _rows(q, k, v, n, lo, sink):
    """fp64 attention of rows q [R,D] over k, v [N,D]: row i sees lo[i] <= j < n[i] and the sink logit sink[i]; no key: 0."""
    R, D = q.shape
    out = torch.zeros(R, D, dtype=torch.float64)
    top = int(n.max()) if R else 0
    if top <= 0:
        return out
    j = torch.arange(top)[None, :]
    s = (q.double() @ k[:top].double().T / D ** 0.5).masked_fill((j >= n[:, None]) | (j < lo[:, None]), NEG_INF)
    live = n > lo
    lse = torch.logaddexp(torch.logsumexp(s[live], dim=-1), sink[live].double())
    out[live] = torch.exp(s[live] - lse[:, None]) @ v[:top].double()
    return out


def mapped(q, k_pages, v_pages, block_table, lens, cu, W, sinks, defect=None):
    """O fp64 of the packed q [total_q,Hq,D] (a decode's [B,T,Hq,D] is packed with cu = [0, T, 2 T, ...]) as the kernels' walk produces it, with
    `defect` in (None, "shift", "sink8", "slot"). Rows never written are 0."""
    W = INT_MAX if W is None else W
    total_q, Hq, D = q.shape
    Hkv = k_pages.shape[1]
    G, B = Hq // Hkv, len(cu) - 1
    Nmax = block_table.shape[1] * k_pages.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (k_pages, v_pages))
    c = _pow2(G)
    qf = q.reshape(total_q * Hq, D)
    of = torch.zeros(total_q * Hq, D, dtype=torch.float64)
    snk = torch.full((Hq + 8 * Hkv + 16,), NEG_INF) if sinks is None else torch.cat((sinks.float(), torch.zeros(8 * Hkv + 16)))
    Gs = (1 << c) if defect == "slot" else G
    slots = total_q * G // ROW_TILE + B
    first = [cu[b] * Gs // ROW_TILE + b for b in range(B)]
    for b in range(B):
        T = cu[b + 1] - cu[b]
        R = T * G
        tiles = -(-R // ROW_TILE)
        # the tiles of the sequence that have a slot of the grid which the binary search gives to this sequence
        nxt = [first[x] for x in range(b + 1, B)]
        have = [t for t in range(tiles) if first[b] + t < slots and all(first[b] + t < s for s in nxt)]
        r = torch.cat([torch.arange(t * ROW_TILE, min((t + 1) * ROW_TILE, R)) for t in have]) if have else torch.zeros(0, dtype=torch.int64)
        if not len(r):
            continue
        tok, grp = ((r >> c), (r & ((1 << c) - 1))) if defect == "shift" else (r // G, r % G)
        length = min(max(int(lens[b]), 0), Nmax)
        n = (length - (T - 1 - tok)).clamp(min=0)
        lo = (n - W).clamp(min=0)
        for h in range(Hkv):
            flat = (cu[b] * Hq + h * G) + tok * Hq + grp
            ok = flat < total_q * Hq  # the model stays inside the tensor; the defect on the device would not
            sink = snk[(h * 8 if defect == "sink8" else h * G) + grp]
            of[flat[ok]] = _rows(qf[flat[ok]], k[b, h], v[b, h], n[ok], lo[ok], sink[ok])
    return of.view(total_q, Hq, D)


def away(ref, bound, o):
    fin = torch.isfinite(ref)
    return float((o[fin] - ref[fin]).abs().max()) / bound
