"""Helpers of the sliding-window paged attention tests (tests/test_paged_window_surface.py, tests/test_gpu_paged_window_attention.py): Python
mirrors of paged::multi_window_plan and of the split arithmetic of csrc/flash_attn_decode_paged_multi_window_bf16.cuh, mirrors of the two describe
texts, the fp64 reference and the bf16 emulation with the window's mask, and the table with stale entries.

The query token at absolute position p = len_b - T_b + t sees key j iff max(0, p - W + 1) <= j <= p. With n(b,t) = p + 1 the keys the unwindowed
entries show it (prefill_reference.visible), that is lo(b,t) <= j < n(b,t), lo = max(0, n - W).

The criteria are those of the bf16 tests, no new tolerance: O is held to paged_bf16_reference.o_bound(emul, ref), where the emulation is
paged_bf16_reference.emul_rows with a per-row lower bound (emul_rows below: the same six steps, the mask has two sides); LSE to
decode_reference.lse_tol; -inf rows and zero rows exactly.

Largest err / bound of O seen on an MI355X over every case of tests/test_gpu_paged_window_attention.py: prefill 0.327 (D = 64, G = 1, page 16,
context 63, W = 65), decode with one split 0.251 (D = 128, T = 8, G = 4, W = 33), with three splits 0.092 (W = 1000). LSE: at most 0.0002 of
lse_tol.

A plain module: nothing here is collected."""
import torch

import decode_reference as dr
import multi_decode_reference as mr
import paged_bf16_reference as br
import paged_decode_reference as pr
import prefill_reference as pf

ROW_TILE, KEY_STEP = br.ROW_TILE, br.KEY_STEP  # the prefill's tile and key step: 128 rows, 64 keys
MULTI_KEY_STEP = mr.KEY_STEP                   # the decode's key step: 128
LOG2E = br.LOG2E
INT_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------- plan and split arithmetic

def unit(page):
    """U of the decode: what a chunk and a sequence's base are multiples of."""
    return max(page, MULTI_KEY_STEP)


def span(T, max_pages, page, W):
    """min(Nmax, round_up(W + T - 1, U) + U): the keys between a sequence's base and its length, at most."""
    U = unit(page)
    return min(max_pages * page, -(-(W + T - 1) // U) * U + U)


def plan(B, T, Hq, Hkv, max_pages, page, D, W):
    """(splits, chunk, workspace_bytes) as cln_fa2_decode_paged_multi_window_bf16_plan computes them: fa2d::split_plan on B Hkv workgroups per
    split over the span, the chunk a multiple of U."""
    n, U, bk = span(T, max_pages, page, W), unit(page), B * Hkv
    want = 1
    if bk < dr.TARGET_WORKGROUPS and n > dr.MIN_CHUNK:
        want = min(-(-dr.TARGET_WORKGROUPS // bk), n // dr.MIN_CHUNK, dr.MAX_SPLITS)
    chunk = -(-(-(-n // want)) // U) * U
    splits = -(-n // chunk)
    return splits, chunk, mr.workspace_bytes(B, T, Hq, splits, D)


def lo_min(n, T, W):
    """The lower edge of the first of the T new tokens of a sequence of n keys: max(0, n - T - W + 1)."""
    return max(0, n - T - W + 1)


def base(n, T, W, U):
    """align_down(lo_min, U): where the first split of the decode starts, and below which neither family reads (U = max(page, key step))."""
    return lo_min(n, T, W) // U * U


def live_splits(n, T, W, page, C):
    """ceil((len - base) / C): the splits of a sequence of n keys that hold a key."""
    return -(-(n - base(n, T, W, unit(page))) // C)


# ---------------------------------------------------------------------------------------------------- describe texts

def describe_prefill_text(B, total_q, Hq, Hkv, max_pages, page, D, W):
    """The text of cln_fa2_prefill_paged_varlen_window_bf16_describe for a supported shape."""
    G = Hq // Hkv
    S = total_q * G // ROW_TILE + B
    reach = min(W + ROW_TILE // G + 2 * KEY_STEP, max_pages * page)
    return ("fa2_prefill_paged_varlen_window_bf16_mfma<D=%d,G=%d> B=%d total_q=%d page=%d rows=%d keys=%d W=%d: one launch, no "
            "workspace; %d workgroups of 256 threads (%d KV heads x %d slots = total_q G / %d + B, at most B of them empty), "
            "sequence b owns the slots from cu_q[b] G / %d + b, found by binary search over the device-side offsets; a slot is a tile "
            "of %d of the T_b G query rows t G + g of its sequence, 32 rows per wave, and walks the keys from the step that holds the "
            "lower edge p - W + 1 of its first token to the causal edge of its last in steps of %d, a span of at most %d keys "
            "whatever the length; K and V rows through the block table to LDS once per workgroup, no table entry and no row below "
            "that first step; S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, V through ds_read_b64_tr_b16, fp32 scores, "
            "window and causal mask by select on the steps that cross an edge, online softmax, no split over the keys (S=1, C=the "
            "span); deterministic"
            % (D, G, B, total_q, page, ROW_TILE, KEY_STEP, W, Hkv * S, Hkv, S, ROW_TILE, ROW_TILE, ROW_TILE, KEY_STEP, reach))


def describe_multi_text(B, T, Hq, Hkv, max_pages, page, D, W):
    """The text of cln_fa2_decode_paged_multi_window_bf16_describe for a supported shape."""
    G = Hq // Hkv
    tiles = -(-T * G // mr.TILE_ROWS)
    S, C, ws = plan(B, T, Hq, Hkv, max_pages, page, D, W)
    text = ("fa2_decode_paged_multi_window_bf16_mfma<D=%d,MT=%d> T=%d G=%d W=%d span=%d S=%d C=%d page=%d: the S splits of C keys divide the "
            "span from base = align_down(max(0, len - T - W + 1), %d) on, no table entry and no row below base; 4 waves split the %d-key "
            "steps, K rows through the block table straight to MFMA fragments, V rows through a transposed LDS read, each row loaded once "
            "for the %d query rows (T x G, %d tiles of 16) of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, fp32 "
            "scores, window and causal mask by select, online softmax"
            % (D, tiles, T, G, W, span(T, max_pages, page, W), S, C, page, unit(page), MULTI_KEY_STEP, T * G, tiles))
    if S > 1:
        text += ("; then fa2_decode_combine_window_bf16_rows<D=%d> merges the live splits ceil((len - base) / C) of a query row by log-sum-exp in "
                 "ascending order (workspace %d bytes)" % (D, ws))
    return text + "; deterministic"


# ---------------------------------------------------------------------------------------------------- reference and emulation

def emul_rows(q, k, v, vis, lo):
    """paged_bf16_reference.emul_rows with a lower bound: query r sees the keys lo[r] <= j < vis[r]. O_emul fp64 [R,D] holding bf16 values."""
    R, D = q.shape
    out = torch.zeros(R, D, dtype=torch.float64)
    top = int(max(vis)) if len(vis) else 0
    if top == 0:
        return out
    vist, lot = torch.tensor(list(vis), dtype=torch.int64), torch.tensor(list(lo), dtype=torch.int64)
    live = vist > lot
    j = torch.arange(top)[None, :]
    s = (q.double() @ k[:top].double().T).float() * torch.tensor(LOG2E / D ** 0.5, dtype=torch.float32)  # 1: fp64 scores, cast to fp32, scaled there
    s = s.masked_fill((j >= vist[:, None]) | (j < lot[:, None]), float("-inf"))[live]
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)                                                # 2: fp32, the row's final maximum
    lsum = p.sum(dim=-1, dtype=torch.float32)                                                              # 5: fp32 row sum of the unrounded P
    o = p.bfloat16().double() @ v[:top].double()                                                           # 3, 4
    out[live] = (o / lsum.double()[:, None]).float().bfloat16().double()                                   # 5, 6
    return out


def _sequence(qb, kd, vd, vis, W):
    """(O fp64 [T,Hq,D], LSE fp64 [T,Hq], O_emul fp64 [T,Hq,D]) of one sequence: qb bf16 [T,Hq,D], kd / vd its gathered dense cache [Hkv,N,D],
    vis [T] = n(b,t). The fp64 reference is the masked softmax over the dense cache, written out."""
    T, Hq, D = qb.shape
    G = Hq // kd.shape[0]
    vis = [int(x) for x in vis]
    lo = [max(0, n - W) for n in vis]
    O = torch.zeros(T, Hq, D, dtype=torch.float64)
    L = torch.full((T, Hq), float("-inf"), dtype=torch.float64)
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
        s = (qb[live, h].double() @ kh.T / D ** 0.5).masked_fill(hidden, float("-inf"))
        lse = torch.logsumexp(s, dim=-1)
        O[live, h] = torch.exp(s - lse[:, None]) @ vh
        L[live, h] = lse
        E[:, h] = emul_rows(qb[:, h], kd[h // G], vd[h // G], vis, lo)
    return O, L, E


def prefill(q, k_pages, v_pages, block_table, lens, cu, W):
    """(O [total_q,Hq,D], LSE [total_q,Hq], O_emul) of the packed q, all fp64; NaN in the rows of no sequence."""
    Nmax = block_table.shape[1] * k_pages.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (k_pages, v_pages))
    O = torch.full(q.shape, float("nan"), dtype=torch.float64)
    L = torch.full(q.shape[:2], float("nan"), dtype=torch.float64)
    E = torch.full(q.shape, float("nan"), dtype=torch.float64)
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        if hi > lo:
            O[lo:hi], L[lo:hi], E[lo:hi] = _sequence(q[lo:hi], k[b], v[b], pf.visible([lens[b]], hi - lo, Nmax)[0].tolist(), W)
    return O, L, E


def decode(q, k_pages, v_pages, block_table, lens, W):
    """(O [B,T,Hq,D], LSE [B,T,Hq], O_emul), all fp64."""
    B, T = q.shape[:2]
    Nmax = block_table.shape[1] * k_pages.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (k_pages, v_pages))
    vis = mr.visible(lens, T, Nmax)
    got = [_sequence(q[b], k[b], v[b], vis[b * T:(b + 1) * T], W) for b in range(B)]
    return tuple(torch.stack([g[i] for g in got]) for i in range(3))


# ---------------------------------------------------------------------------------------------------- stale table entries

def stale_table(block_table, lens, Ts, W, page, key_step, to_page):
    """(table, redirected): every entry of a logical page that ends at or before align_down(max(0, len_b - T_b - W + 1), max(page, key_step))
    points at `to_page` -- a VALID pool page, which the caller has filled with NaN; the count of entries that were live pages before."""
    bt = block_table.clone()
    Nmax = bt.shape[1] * page
    n = 0
    for b, T in enumerate(Ts):
        ln = min(max(int(lens[b]), 0), Nmax)
        stale = base(ln, T, W, max(page, key_step)) // page
        bt[b, :stale] = to_page
        n += stale
    return bt, n
