"""Reference for the paged KV-cache append tests (tests/test_kv_append_paged_surface.py proves it against brute force,
tests/test_gpu_kv_append_paged.py uses it): cuda_learn_notes_amd.kv_append_paged / cln_kv_append_paged (csrc/kv_append_paged.cuh) on the CPU.
The pool rows are copied by Python loops over (b, t); the rotation is in float64 from the fp16 inputs and the fp32 table values. The error bound
of the GPU tests is derived here, not measured. A plain module: nothing here is collected."""
from collections import namedtuple

import torch

MODES = {"none": 0, "half": 1, "interleaved": 2}

# k_pages, v_pages: the pools after the call (fp16; a rotated K row holds the fp64 value rounded once -- compare those rows through k_rot and the
# bound, everything else bit for bit). k_live: bool [P, page], the K / V pool rows the call writes. k_rot, k_mag: fp64 [B,T,Hkv,D], the exact
# rotated K rows and |x1 c| + |x2 s| (resp. |x1 s| + |x2 c|) of every element, zero for tokens that are not live; q_rot, q_mag: the same for q
# [B,T,Hq,D] (q_rot of a token that is not live is the zero row the kernel writes), None without q. live: the list of live (b, t).
Result = namedtuple("Result", "k_pages v_pages k_live k_rot k_mag q_rot q_mag live")


def rotate(x, row, mode):
    """(rotated, magnitude) in float64 of rows x [..., D] by the table row [D] = cos for i < D/2, then sin: pair (x1, x2) becomes
    (x1 c - x2 s, x1 s + x2 c); magnitude = |x1 c| + |x2 s| resp. |x1 s| + |x2 c|, what the bound's fp32 term scales with. mode 1 pairs
    (i, i + D/2), mode 2 pairs (2i, 2i + 1), mode 0 returns x."""
    x = x.double()
    if mode == 0:
        return x, x.abs()
    D = x.shape[-1]
    c, s = row[:D // 2].double(), row[D // 2:].double()
    x1, x2 = (x[..., :D // 2], x[..., D // 2:]) if mode == 1 else (x[..., 0::2], x[..., 1::2])
    a, b = x1 * c - x2 * s, x1 * s + x2 * c
    ma, mb = (x1 * c).abs() + (x2 * s).abs(), (x1 * s).abs() + (x2 * c).abs()
    if mode == 1:
        return torch.cat((a, b), dim=-1), torch.cat((ma, mb), dim=-1)
    return torch.stack((a, b), dim=-1).flatten(-2), torch.stack((ma, mb), dim=-1).flatten(-2)


def ref_append(k_new, v_new, k_pages, v_pages, block_table, lens, q, table, mode):
    """The call on the CPU. k_new, v_new fp16 [B,T,Hkv,D]; pools fp16 [P,Hkv,page,D] (not modified: the result holds copies); block_table int
    [B,max_pages]; lens: B Python ints, any value; q fp16 [B,T,Hq,D] or None; table fp32 [max_pos,D] or None; mode 0, 1 or 2."""
    B, T, Hkv, D = k_new.shape
    P, _, page, _ = k_pages.shape
    cap = block_table.shape[1] * page
    kp, vp = k_pages.clone(), v_pages.clone()
    k_live = torch.zeros(P, page, dtype=torch.bool)
    k_rot, k_mag = torch.zeros(B, T, Hkv, D, dtype=torch.float64), torch.zeros(B, T, Hkv, D, dtype=torch.float64)
    q_rot = q_mag = None
    if q is not None:
        q_rot, q_mag = torch.zeros(q.shape, dtype=torch.float64), torch.zeros(q.shape, dtype=torch.float64)
    live = []
    for b in range(B):
        for t in range(T):
            pos = int(lens[b]) - T + t
            if not (0 <= pos < cap) or (mode != 0 and pos >= table.shape[0]):
                continue
            live.append((b, t))
            pg, row = int(block_table[b, pos // page]), pos % page
            assert 0 <= pg < P and not bool(k_live[pg, row]), "the caller's contract: live entries in [0, P), no page named twice"
            k_live[pg, row] = True
            trow = table[pos] if mode != 0 else None
            k_rot[b, t], k_mag[b, t] = rotate(k_new[b, t], trow, mode)
            kp[pg, :, row] = k_new[b, t] if mode == 0 else k_rot[b, t].to(torch.float16)
            vp[pg, :, row] = v_new[b, t]
            if q is not None:
                q_rot[b, t], q_mag[b, t] = rotate(q[b, t], trow, mode)
    return Result(kp, vp, k_live, k_rot, k_mag, q_rot, q_mag, live)


def bound(r, mag):
    """What an output element may differ from its exact value r = x1 c - x2 s (or x1 s + x2 c) by, with mag = |x1 c| + |x2 s|:
        2^-11 |r|     the one rounding to fp16 (round to nearest: half an ulp of a normal number),
      + 2^-25         its floor in the subnormal range (half of the spacing 2^-24),
      + 2^-22 mag     a generous cover of the fp32 arithmetic in front of it: three roundings of 2^-24 relative each (two products, one sum; with
                      a fused multiply-add two), and the double rounding fp64 -> fp32 -> fp16, which moves the fp16 result by at most the fp32
                      error. fp16 inputs and fp32 table values are exact in fp32."""
    return 2.0 ** -11 * r.abs() + 2.0 ** -25 + 2.0 ** -22 * mag
