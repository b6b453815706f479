"""Helpers of the tests of the latent cache in DeepSeek-V3.2's own FP8 row of 656 bytes: the layout written from the contract,
the per-tile quantiser in torch fp32 operations, the dequantised bf16 pool c[d] = bf16(fp32(code[d]) * scale[d // 128]) on which
paged_mla_sparse_reference.decode_sparse is the decode's fp64 reference, and pools for the decode tests. Nothing here is collected."""
import functools
import random

import torch

import fp8_kv_reference as fk
import mla_index_reference as ix
import paged_mla_sparse_reference as sp

BF, F8 = torch.bfloat16, torch.float8_e4m3fn
ROW, DC, DR, TILE, TILES = 656, 512, 64, 128, 4


def views(pool):
    """(codes e4m3fn [P,page,512], scales fp32 [P,page,4], k_pe bf16 [P,page,64]) of pool uint8 [P,page,656], views of its storage."""
    assert pool.dtype == torch.uint8 and pool.shape[2] == ROW and pool.is_contiguous()
    return pool[..., :DC].view(F8), pool[..., DC:DC + 4 * TILES].view(torch.float32), pool[..., DC + 4 * TILES:].view(BF)


def nan_pool(P, page):
    """A pool in which no token is stored: every code byte 0x7F (NaN), every scale NaN, every k_pe NaN."""
    pool = torch.empty(P, page, ROW, dtype=torch.uint8)
    codes, scales, k_pe = views(pool)
    codes.view(torch.uint8).fill_(0x7F)
    scales.fill_(float("nan"))
    k_pe.fill_(float("nan"))
    return pool


def quantise(c, pow2):
    """(codes e4m3fn [n,512], scales fp32 [n,4]) of bf16 rows c [n,512]: the formula of the append, all in fp32."""
    t = c.float().view(-1, TILES, TILE)
    s = t.abs().amax(dim=-1).clamp_min(torch.tensor(1e-4, dtype=torch.float32)) / torch.tensor(448.0, dtype=torch.float32)
    if pow2:
        b = s.view(torch.int32)
        s = torch.where((b & 0x007FFFFF) != 0, (b & 0x7F800000) + 0x00800000, b).view(torch.float32)
    return fk.quantize(t, s[..., None]).view(-1, DC), s


def dequantised(pool):
    """bf16 [P,page,576]: what a stored row means, the pool fa2_decode_paged_mla_sparse_bf16 gives the same bits on."""
    codes, scales, k_pe = views(pool)
    return torch.cat(((codes.float() * scales.repeat_interleave(TILE, -1)).bfloat16(), k_pe), -1)


def append_ref(pool, bt, lens_after, cu, c_new, k_pe_rot, pow2):
    """The pool bytes after kv_append_paged_mla_bf16_fp8_tile, k_pe_rot the rotated rows; rows placed as mla_index_reference.append_ref does."""
    out = pool.clone()
    codes, scales, k_pe = views(out)
    P, page = pool.shape[:2]
    c, Ts = ix.append_clamped(cu, c_new.shape[0])
    qc, qs = quantise(c_new, pow2)
    for b in range(len(lens_after)):
        for i in range(Ts[b]):
            pos = lens_after[b] - Ts[b] + i
            if 0 <= pos < bt.shape[1] * page and 0 <= int(bt[b, pos // page]) < P:
                at = (int(bt[b, pos // page]), pos % page)
                codes.view(torch.uint8)[at], scales[at], k_pe[at] = qc[c[b] + i].view(torch.uint8), qs[c[b] + i], k_pe_rot[c[b] + i]
    return out


@functools.lru_cache(maxsize=None)
def latent(n, seed):
    """(c bf16 [n,512], k_pe bf16 [n,64]), never modified: tile k of token i scaled by 2^((3 i + 5 k) mod 13 - 6), k_pe at 2^-9."""
    g = torch.Generator().manual_seed(seed)
    e = (3 * torch.arange(n)[:, None] + 5 * torch.arange(TILES)[None, :]) % 13 - 6
    c = torch.randn(n, TILES, TILE, generator=g) * sp.SCALE * torch.exp2(e.float())[..., None]
    return c.view(n, DC).to(BF), (torch.randn(n, DR, generator=g) * 2.0 ** -9).to(BF)


def listed(lens, T, Nmax, indices):
    """Per sequence the sorted positions that a list [B,T,topk] names as a valid slot."""
    vis = sp.visible(lens, T, Nmax)
    return [sorted({p for t in range(T) for _, p in sp.valid_slots(indices[b, t], vis[b][t])}) for b in range(len(lens))]


def listed_pool(c, k_pe, page, lens, positions, seed=0, pow2=False):
    """(pool uint8 [P,page,656], block_table int32 [B,max_pages]) of dense c [B,Nmax,512], k_pe [B,Nmax,64] holding ONLY the rows positions[b]:
    every other row, and the page P - 1 that the table entries past ceil(len_b / page) name, is NaN codes, NaN scales and NaN k_pe."""
    B, Nmax = c.shape[:2]
    max_pages = Nmax // page
    live = [-(-min(max(n, 0), Nmax) // page) for n in lens]
    P = sum(live) + 3
    perm = random.Random(seed).sample(range(P - 1), sum(live))
    bt = torch.full((B, max_pages), P - 1, dtype=torch.int32)
    pool = nan_pool(P, page)
    codes, scales, pe = views(pool)
    for b in range(B):
        bt[b, :live[b]] = torch.tensor(perm[sum(live[:b]):sum(live[:b + 1])], dtype=torch.int32)
        pos = positions[b]
        if pos:
            pt = torch.tensor(pos)
            qc, qs = quantise(c[b, pt], pow2)
            at = (bt[b, pt // page].long(), pt % page)
            codes.view(torch.uint8)[at], scales[at], pe[at] = qc.view(torch.uint8), qs, k_pe[b, pt]
    return pool, bt


TH, TOPKS = [(1, 1), (1, 16), (2, 40), (1, 128)], [1, 63, 64, 65, 130, 1024]  # one split up to 130; 1024: 4 splits of 256
LENS, NMAX = [0, 40, 1500], 2048    # a length of 0, one below every topk from 63 on, one that fills two thirds of 1024 slots
CORNERS = {(1, 1, 16, 1), (1, 128, 64, 130), (2, 40, 16, 1024), (1, 128, 64, 1024)}  # (T, Hq, page, topk) of the fp64 parity


@functools.lru_cache(maxsize=None)
def case(T, Hq, page, topk):
    """(q bf16 [3,T,Hq,576], LENS, (pool, block_table), indices int32 [3,T,topk]); q x 4 so that the softmax is not flat."""
    g = torch.Generator().manual_seed(1000 * T + 10 * Hq + page + topk)
    q = (torch.randn(len(LENS), T, Hq, sp.DK, generator=g) * sp.SCALE * 4).to(BF)
    c, k_pe = latent(len(LENS) * NMAX, 5)
    idx = sp.sample_indices(LENS, T, NMAX, topk, seed=7 * T + Hq + page + topk)
    pool = listed_pool(c.view(len(LENS), NMAX, DC), k_pe.view(len(LENS), NMAX, DR), page, LENS, listed(LENS, T, NMAX, idx), seed=topk)
    return q, LENS, pool, idx
