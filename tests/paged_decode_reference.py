"""References for the paged decode attention tests (tests/test_fa2_decode_paged_surface.py proves them, tests/test_gpu_fa2_decode_paged.py uses
them): the gather of a paged cache into the dense one, the fp64 reference through the unmodified decode_reference.ref_decode, a Python mirror of
the plan of csrc/flash_attn_decode_paged.hip, and the builder of the shuffled, poisoned page pools the GPU tests run on. The tolerances are
decode_reference.fa_tol / lse_tol. A plain module: nothing here is collected."""
import torch

import decode_reference as dr

GROUPS = (1, 2, 4, 8)
PAGES = (16, 32, 64, 128, 256)


def plan(B, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) as cln_fa2_decode_paged_plan computes them: the decode plan on B Hkv workgroups per split (a workgroup
    serves a whole group of query heads) with the chunk a multiple of max(page, key step)."""
    Nmax, unit, bk = max_pages * page, max(page, dr.key_step(D)), B * Hkv
    want = 1
    if bk < dr.TARGET_WORKGROUPS and Nmax > dr.MIN_CHUNK:
        want = min(-(-dr.TARGET_WORKGROUPS // bk), Nmax // dr.MIN_CHUNK, dr.MAX_SPLITS)
    chunk = -(-(-(-Nmax // want)) // unit) * unit
    splits = -(-Nmax // chunk)
    return splits, chunk, dr.workspace_bytes(B, Hq, splits, D)


def gather(pages, block_table, lens):
    """Dense [B,Hkv,Nmax,D] from pages [P,Hkv,page,D]: logical row j of sequence b = row j % page of page block_table[b, j // page]. Only the
    entries 0 .. ceil(len_b / page) - 1 are followed (len_b clamped to [0, Nmax]); every other row is zero."""
    P, Hkv, page, D = pages.shape
    B, max_pages = block_table.shape
    out = torch.zeros(B, Hkv, max_pages * page, D, dtype=pages.dtype)
    for b in range(B):
        n = min(max(int(lens[b]), 0), max_pages * page)
        for i in range(-(-n // page)):
            out[b, :, i * page:(i + 1) * page] = pages[int(block_table[b, i])]
    return out


def ref_decode_paged(q, k_pages, v_pages, block_table, lens):
    """fp64 (O [B,Hq,D], LSE [B,Hq]): query head h attends KV head h // G of the gathered cache, through decode_reference.ref_decode."""
    Hq, Hkv = q.shape[1], k_pages.shape[1]
    G = Hq // Hkv
    assert G * Hkv == Hq
    k, v = (gather(t.cpu(), block_table.cpu(), lens).repeat_interleave(G, dim=1) for t in (k_pages, v_pages))
    return dr.ref_decode(q, k, v, lens)


def make_pool(k, v, page, lens, order="shuffle", seed=0, extra=0, fill=float("nan")):
    """The paged form of dense caches k, v [B,Hkv,Nmax,D] (Nmax a multiple of page) for the lengths `lens`, as the GPU tests want it:
    P = 3 live // 2 + 1 + extra pages (+ 1 poison page), the live pages of the sequences interleaved and then placed by a seeded permutation
    (order="identity": in interleaved order), every page no live entry names -- the poison page among them -- filled with `fill`, and every table
    entry past ceil(len_b / page) pointing at the poison page. Returns (k_pages, v_pages, block_table int32 [B,max_pages])."""
    B, Hkv, Nmax, D = k.shape
    max_pages = Nmax // page
    assert max_pages * page == Nmax
    live = [(i, b) for i in range(max_pages) for b in range(B) if i < -(-min(max(int(lens[b]), 0), Nmax) // page)]
    P = 3 * len(live) // 2 + 2 + extra
    poison = P - 1
    g = torch.Generator().manual_seed(seed)
    slots = torch.randperm(P - 1, generator=g).tolist() if order == "shuffle" else list(range(P - 1))
    kp = torch.full((P, Hkv, page, D), fill, dtype=k.dtype)
    vp = torch.full((P, Hkv, page, D), fill, dtype=v.dtype)
    bt = torch.full((B, max_pages), poison, dtype=torch.int32)
    for slot, (i, b) in zip(slots, live):
        kp[slot] = k[b, :, i * page:(i + 1) * page]
        vp[slot] = v[b, :, i * page:(i + 1) * page]
        bt[b, i] = slot
    return kp, vp, bt
