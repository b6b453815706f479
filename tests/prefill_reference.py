"""References for the paged prefill attention tests (tests/test_fa2_prefill_paged_surface.py proves them, tests/test_gpu_fa2_prefill_paged.py uses
them): the tile geometry of csrc/flash_attn_prefill_paged.cuh, a Python mirror of the describe text of csrc/flash_attn_prefill_paged.hip, and the
fp64 reference -- the cache gathered once with the unmodified paged_decode_reference.gather, then ONE masked softmax per (b, h) over [T, top]
scores; the cache is not copied per query token. Pools come from paged_decode_reference.make_pool; the tolerances are decode_reference.fa_tol /
lse_tol. A plain module: nothing here is collected."""
import torch

import paged_decode_reference as pr

ROW_TILE = 128  # query rows r = t G + g of one workgroup of fa2pp::fa2_prefill_paged_kernel: 4 waves x 32 rows
KEY_STEP = 64   # keys per workgroup step, for both head dims
WAVE_ROWS = 32
MFMA_ROWS = 16


def tiles(T, G):
    """Workgroups per (sequence, KV head)."""
    return -(-T * G // ROW_TILE)


def describe_text(B, T, Hq, Hkv, max_pages, page, D):
    """The text of cln_fa2_prefill_paged_describe for a supported shape."""
    G = Hq // Hkv
    nt = tiles(T, G)
    return ("fa2_prefill_paged<D=%d,G=%d> T=%d page=%d rows=%d keys=%d: one launch, no workspace; %d workgroups of 256 threads (%d "
            "(sequence, KV head) pairs x %d tiles of %d of the %d query rows t G + g, 32 rows per wave), each walks the keys below "
            "the causal edge of its last token in steps of %d, K and V rows through the block table to LDS once per workgroup, S^T = K "
            "Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16, V through ds_read_b64_tr_b16, fp32 scores, causal mask by select on the "
            "steps that cross the edge, online softmax, no split over the keys; deterministic"
            % (D, G, T, page, ROW_TILE, KEY_STEP, B * Hkv * nt, B * Hkv, nt, ROW_TILE, T * G, KEY_STEP))


def visible(lens, T, Nmax):
    """int64 [B,T]: n(b,t) = len_b - (T - 1 - t) with len_b = clamp(lens[b], 0, Nmax), never fewer than 0."""
    n = torch.tensor([min(max(int(x), 0), Nmax) for x in lens], dtype=torch.int64)
    return (n[:, None] - (T - 1 - torch.arange(T, dtype=torch.int64))[None, :]).clamp_(min=0)


def ref_prefill_paged(q, k_pages, v_pages, block_table, lens):
    """fp64 (O [B,T,Hq,D], LSE [B,T,Hq]): query (b, t, h) attends the first n(b,t) keys of KV head h // G of sequence b's gathered cache;
    n(b,t) = 0 gives O = 0 and LSE = -inf."""
    B, T, Hq, D = q.shape
    Hkv = k_pages.shape[1]
    G = Hq // Hkv
    assert G * Hkv == Hq
    Nmax = block_table.shape[1] * k_pages.shape[2]
    vis = visible(lens, T, Nmax)
    k, v = (pr.gather(t.cpu(), block_table.cpu(), lens) for t in (k_pages, v_pages))  # [B,Hkv,Nmax,D], once
    qd = q.cpu().double().view(B, T, Hkv, G, D)
    O = torch.zeros(B, T, Hq, D, dtype=torch.float64)
    L = torch.full((B, T, Hq), float("-inf"), dtype=torch.float64)
    for b in range(B):
        top = int(vis[b].max())  # no query of b sees a row at or past this: what lies there (NaN in the tests) is never touched
        live = vis[b] > 0
        if top == 0:
            continue
        mask = torch.arange(top)[None, :] < vis[b][:, None]  # [T, top]
        kb, vb = k[b, :, :top].double(), v[b, :, :top].double()
        for h in range(Hq):
            s = (qd[b, :, h // G, h % G] @ kb[h // G].T) / D ** 0.5  # [T, top]
            s = s.masked_fill(~mask, float("-inf"))[live]
            lse = torch.logsumexp(s, dim=-1)
            O[b, live, h] = torch.exp(s - lse[:, None]) @ vb[h // G]
            L[b, live, h] = lse
    return O, L
