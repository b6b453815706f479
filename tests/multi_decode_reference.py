"""References for the multi-token paged decode attention tests (tests/test_fa2_decode_paged_multi_surface.py proves them,
tests/test_gpu_fa2_decode_paged_multi.py uses them): a Python mirror of the plan of csrc/flash_attn_decode_paged_multi.hip and the fp64 reference,
built on the unmodified paged_decode_reference.gather and decode_reference.ref_decode -- every (b, t) is a sequence of its own with the length
n(b,t) = len_b - (T - 1 - t) clamped at 0, over the gathered cache of b. Pools come from paged_decode_reference.make_pool; the tolerances are
decode_reference.fa_tol / lse_tol. A plain module: nothing here is collected."""
import torch

import decode_reference as dr
import paged_decode_reference as pr

KEY_STEP = 128  # keys per workgroup step of fa2pm::fa2_decode_paged_multi_kernel: 4 waves x 32 keys, for both head dims
MAX_T = 8
TILE_ROWS = 16  # query rows of one MFMA M tile


def plan(B, T, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) as cln_fa2_decode_paged_multi_plan computes them: the paged decode plan on B Hkv workgroups per split (a
    workgroup serves all T G query rows of its KV head, so T does not enter the split) with the chunk a multiple of max(page, KEY_STEP)."""
    Nmax, unit, bk = max_pages * page, max(page, KEY_STEP), B * Hkv
    want = 1
    if bk < dr.TARGET_WORKGROUPS and Nmax > dr.MIN_CHUNK:
        want = min(-(-dr.TARGET_WORKGROUPS // bk), Nmax // dr.MIN_CHUNK, dr.MAX_SPLITS)
    chunk = -(-(-(-Nmax // want)) // unit) * unit
    splits = -(-Nmax // chunk)
    return splits, chunk, workspace_bytes(B, T, Hq, splits, D)


def workspace_bytes(B, T, Hq, splits, D):
    """fp32 O partials [B T Hq][S][D] and (m, l) pairs [B T Hq][S][2]; nothing for one split."""
    return B * T * Hq * splits * (D + 2) * 4 if splits > 1 else 0


def visible(lens, T, Nmax):
    """n(b,t) for every (b, t), row-major in (b, t): len_b = clamp(lens[b], 0, Nmax) counts the T newest tokens; query t sees the keys
    j < len_b - (T - 1 - t), never fewer than 0."""
    out = []
    for n in lens:
        n = min(max(int(n), 0), Nmax)
        out += [max(n - (T - 1 - t), 0) for t in range(T)]
    return out


def ref_decode_paged_multi(q, k_pages, v_pages, block_table, lens):
    """fp64 (O [B,T,Hq,D], LSE [B,T,Hq]): query (b, t, h) attends the first n(b,t) keys of KV head h // G of sequence b's gathered cache."""
    B, T, Hq, D = q.shape
    Hkv = k_pages.shape[1]
    G = Hq // Hkv
    assert G * Hkv == Hq
    Nmax = block_table.shape[1] * k_pages.shape[2]
    vis = visible(lens, T, Nmax)
    top = max(1, max(vis))  # no query sees a row at or past this: the copies below stop there
    # [B,Hq,top,D], then one copy per query token: sequence b T + t of the single-query reference
    k, v = (pr.gather(t.cpu(), block_table.cpu(), lens)[:, :, :top].repeat_interleave(G, dim=1).repeat_interleave(T, dim=0) for t in (k_pages, v_pages))
    O, L = dr.ref_decode(q.reshape(B * T, Hq, D), k, v, vis)
    return O.view(B, T, Hq, D), L.view(B, T, Hq)
