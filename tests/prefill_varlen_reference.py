"""References for the packed variable-length paged prefill / append tests (tests/test_fa2_prefill_paged_varlen_surface.py proves them,
tests/test_gpu_fa2_prefill_paged_varlen.py and tests/test_gpu_kv_append_paged_varlen.py use them): the slot mapping of
csrc/flash_attn_prefill_paged_varlen.cuh in Python, mirrors of the two describe texts, and the references -- prefill_reference.ref_prefill_paged
and kv_append_reference.ref_append called once per sequence with B = 1, T = T_b, the table row and the length of that sequence, the results
concatenated. No new numerics enter. A plain module: nothing here is collected."""
import torch

import kv_append_reference as kr
import prefill_reference as pf

ROW_TILE, KEY_STEP = pf.ROW_TILE, pf.KEY_STEP

# the per-sequence token counts of the GPU tests: (Hkv, G, page, max_pages), T
CASES = [((1, 4, 32, 32), [40, 0, 1, 33, 130]), ((2, 1, 16, 40), [128, 1, 129]), ((1, 8, 64, 8), [16, 17, 0, 2]), ((1, 2, 256, 2), [200, 64])]


def cu_of(T, first=0):
    """The offsets [B+1] of the token counts T, the first sequence at packed row `first`."""
    cu = [first]
    for t in T:
        cu.append(cu[-1] + t)
    return cu


def slots(cu, G, total_q=None):
    """(S, first, tiles): the slots per KV head S = total_q G // 128 + B (total_q defaults to cu[B]), the first slot s_b = cu[b] G // 128 + b of
    every sequence and its tile count ceil(T_b G / 128)."""
    B = len(cu) - 1
    total_q = cu[B] if total_q is None else total_q
    first = [cu[b] * G // ROW_TILE + b for b in range(B)]
    tiles = [-(-(cu[b + 1] - cu[b]) * G // ROW_TILE) for b in range(B)]
    return total_q * G // ROW_TILE + B, first, tiles


def slot_owner(cu, G, x):
    """(b, tile) of slot x as the kernel finds it -- the largest b with s_b <= x, tile = x - s_b -- or None for an empty slot."""
    _, first, tiles = slots(cu, G)
    owners = [b for b in range(len(first)) if first[b] <= x]
    if not owners:
        return None
    b = owners[-1]
    return (b, x - first[b]) if x - first[b] < tiles[b] else None


def describe_prefill_text(B, total_q, Hq, Hkv, max_pages, page, D):
    """The text of cln_fa2_prefill_paged_varlen_describe for a supported shape."""
    G = Hq // Hkv
    S = total_q * G // ROW_TILE + B
    return ("fa2_prefill_paged_varlen_mfma<D=%d,G=%d> B=%d total_q=%d page=%d rows=%d keys=%d: one launch, no workspace; %d "
            "workgroups of 256 threads (%d KV heads x %d slots = total_q G / %d + B, at most B of them empty), sequence b owns the "
            "slots from cu_q[b] G / %d + b, found by binary search over the device-side offsets; a slot is a tile of %d of the T_b G "
            "query rows t G + g of its sequence, 32 rows per wave, and walks the keys below the causal edge of its last token in "
            "steps of %d, K and V rows through the block table to LDS once per workgroup, S^T = K Q^T and O^T = V^T P^T on "
            "v_mfma_f32_16x16x32_f16, V through ds_read_b64_tr_b16, fp32 scores, causal mask by select on the steps that cross the "
            "edge, online softmax, no split over the keys; deterministic"
            % (D, G, B, total_q, page, ROW_TILE, KEY_STEP, Hkv * S, Hkv, S, ROW_TILE, ROW_TILE, ROW_TILE, KEY_STEP))


_ROT = ("rows copied bit for bit", "K and q rotated in half-split pairs (i, i + D/2)", "K and q rotated in interleaved pairs (2i, 2i + 1)")


def describe_append_text(B, total_q, Hq, Hkv, max_pages, page, D, mode):
    """The text of cln_kv_append_paged_varlen_describe for a supported shape."""
    rows = 2 * Hkv + (Hq if mode else 0)
    y = -(-rows * (D // 16 if mode == 1 else D // 8) // 256)
    return ("kv_append_paged_varlen_rows<D=%d,ROPE=%d> B=%d total_q=%d page=%d: one launch, no workspace; %d x %d workgroups of 256 "
            "threads (a packed row x the 16-byte pieces of its %d K, %d V and %d q rows), the sequence of a row by binary search over "
            "the device-side offsets, length and table entry through uniform loads, %s%s, plain stores into the pools; deterministic"
            % (D, mode, B, total_q, page, total_q, y, Hkv, Hkv, Hq if mode else 0, _ROT[mode],
               " in fp32 from the cos/sin table with one rounding at the store, V copied" if mode else ""))


def ref_prefill_paged_varlen(q, k_pages, v_pages, block_table, lens, cu):
    """fp64 (O [total_q,Hq,D], LSE [total_q,Hq]) of the packed q [total_q,Hq,D]: per sequence one call of prefill_reference.ref_prefill_paged with
    B = 1 and T = T_b. Rows outside [cu[0], cu[B]) are NaN: they belong to no sequence."""
    total_q, Hq, D = q.shape
    O = torch.full((total_q, Hq, D), float("nan"), dtype=torch.float64)
    L = torch.full((total_q, Hq), float("nan"), dtype=torch.float64)
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        if hi > lo:
            o, l = pf.ref_prefill_paged(q[lo:hi][None], k_pages, v_pages, block_table[b:b + 1], [lens[b]])
            O[lo:hi], L[lo:hi] = o[0], l[0]
    return O, L


def ref_append_varlen(k_new, v_new, k_pages, v_pages, block_table, lens, cu, q, table, mode):
    """kv_append_reference.ref_append per sequence (B = 1, T = T_b), each call on the pools the one before left. Returns (k_pages, v_pages, k_live
    bool [P,page], rows): rows = the list of (packed row, b, pos, k_rot, k_mag, q_rot, q_mag) of the LIVE tokens, the last two None without q; and
    `dead`, the packed rows of the sequences that are not live, as the fifth element."""
    kp, vp = k_pages.clone(), v_pages.clone()
    k_live = torch.zeros(k_pages.shape[0], k_pages.shape[2], dtype=torch.bool)
    rows, dead = [], []
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        if hi == lo:
            continue
        T = hi - lo
        r = kr.ref_append(k_new[lo:hi][None], v_new[lo:hi][None], kp, vp, block_table[b:b + 1], [lens[b]], None if q is None else q[lo:hi][None],
                          table, mode)
        assert not bool((k_live & r.k_live).any()), "the caller's contract: no page named twice"
        kp, vp, k_live = r.k_pages, r.v_pages, k_live | r.k_live
        live = {t for (_, t) in r.live}
        for t in range(T):
            if t in live:
                rows.append((lo + t, b, int(lens[b]) - T + t, r.k_rot[0, t], r.k_mag[0, t], None if q is None else r.q_rot[0, t],
                             None if q is None else r.q_mag[0, t]))
            else:
                dead.append(lo + t)
    return kp, vp, k_live, rows, dead
