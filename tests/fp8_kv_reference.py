"""References for the FP8 (OCP e4m3fn) paged KV cache tests (tests/test_kv_append_paged_fp8_surface.py and
tests/test_fa2_decode_paged_fp8_surface.py prove them on the CPU; tests/test_gpu_kv_append_paged_fp8.py and tests/test_gpu_fa2_decode_paged_fp8.py
use them): the quantiser of cln_kv_append_paged_fp8 in the same fp32 operations, its inverse, the append on the CPU on top of
kv_append_reference, the decode reference on the dequantised pools through paged_decode_reference, a Python mirror of the plan of
csrc/flash_attn_decode_paged_fp8.hip, and the builder of shuffled pools whose unused pages hold the e4m3 NaN byte. The error bound of the rotated
rows is derived here, not measured. A plain module: nothing here is collected."""
from collections import namedtuple

import torch

import decode_reference as dr
import kv_append_reference as kr
import paged_decode_reference as pr

F8 = torch.float8_e4m3fn
FP8_MAX = 448.0
NAN_BYTE = 0x7F


def key_step(D):
    """Keys per workgroup step of the FP8 kernel: 4 waves x 8 loads x (64 lanes / (D / 8) lanes per row)."""
    return 4 * 8 * (64 * 8 // D)


def plan(B, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) as cln_fa2_decode_paged_fp8_plan computes them: paged_decode_reference.plan with the FP8 key step."""
    Nmax, unit, bk = max_pages * page, max(page, key_step(D)), B * Hkv
    want = 1
    if bk < dr.TARGET_WORKGROUPS and Nmax > dr.MIN_CHUNK:
        want = min(-(-dr.TARGET_WORKGROUPS // bk), Nmax // dr.MIN_CHUNK, dr.MAX_SPLITS)
    chunk = -(-(-(-Nmax // want)) // unit) * unit
    splits = -(-Nmax // chunk)
    return splits, chunk, dr.workspace_bytes(B, Hq, splits, D)


def per_head(scale):
    """scale [Hkv] shaped to broadcast against [..., Hkv, rows, D] (a pool or a dense cache): the head axis is third from the end."""
    return scale.reshape(-1, 1, 1)


def quantize(x, scale):
    """e4m3fn of x / scale in the kernel's operations: x exact in fp32, times the fp32 reciprocal of the fp32 scale, clamped to +-448 in fp32,
    rounded to nearest even. scale: a tensor that broadcasts against x."""
    inv = torch.tensor(1.0, dtype=torch.float32) / scale.to(torch.float32)
    return (x.float() * inv).clamp(-FP8_MAX, FP8_MAX).to(F8)


def dequantize(c, scale, dtype=torch.float32):
    """e4m3(c) * scale in `dtype` (fp32: one rounding of 2^-24 relative; float64: exact). scale broadcasts against c."""
    return c.to(dtype) * scale.to(dtype)


def bits(t):
    return t.view(torch.uint8)


# k_pages, v_pages: the pools after the call (e4m3fn; a rotated K row holds quantize() of the fp64 rotation rounded to fp32 -- compare those rows
# through k_rot and bound(), everything else byte for byte). k_live, k_rot, k_mag, q_rot, q_mag, live: as kv_append_reference.Result.
Result = namedtuple("Result", "k_pages v_pages k_live k_rot k_mag q_rot q_mag live")


def ref_append_fp8(k_new, v_new, k_pages, v_pages, block_table, lens, k_scale, v_scale, q, table, mode):
    """cln_kv_append_paged_fp8 on the CPU. k_new, v_new fp16 [B,T,Hkv,D]; pools e4m3fn [P,Hkv,page,D] (not modified: the result holds copies);
    k_scale, v_scale fp32 [Hkv]; the rest as kv_append_reference.ref_append, which decides liveness and rotates."""
    B, T, Hkv, D = k_new.shape
    P, _, page, _ = k_pages.shape
    blank = torch.zeros(P, Hkv, page, D, dtype=torch.float16)
    r = kr.ref_append(k_new, v_new, blank, blank, block_table, lens, q, table, mode)
    kp, vp = bits(k_pages).clone(), bits(v_pages).clone()
    ks, vs = k_scale.reshape(-1, 1), v_scale.reshape(-1, 1)
    for (b, t) in r.live:
        pos = int(lens[b]) - T + t
        pg, row = int(block_table[b, pos // page]), pos % page
        kp[pg, :, row] = bits(quantize(r.k_rot[b, t].float(), ks))  # mode 0 and the unit tables: k_rot is exact in fp32
        vp[pg, :, row] = bits(quantize(v_new[b, t], vs))
    return Result(kp.view(F8), vp.view(F8), r.k_live, r.k_rot, r.k_mag, r.q_rot, r.q_mag, r.live)


def bound(y, scale, mag):
    """What dequantize(byte) may differ from the exact rotated value y by, for |y| <= 448 scale, with mag as kv_append_reference.rotate gives it:
        2^-4 |y|        the one rounding to e4m3 (three mantissa bits: an ulp is at most 2^-3 of the value, round to nearest gives half of it),
      + 2^-10 scale     its floor in the subnormal range (spacing 2^-9 in units of the scale, half of it),
      + 2^-21 mag       a generous cover of the fp32 arithmetic in front of it: three roundings of 2^-24 relative in the rotation (two with a
                        fused multiply-add), one in 1 / scale and one in the product, five in all, each at most 2^-24 mag in units of y; an fp32
                        error that carries the value across a rounding boundary adds no more than itself to the half ulp.
    fp16 inputs and fp32 table values are exact in fp32, and dequantize in float64 is exact."""
    return 2.0 ** -4 * y.abs() + 2.0 ** -10 * scale + 2.0 ** -21 * mag


def ref_decode_paged_fp8(q, k_pages, v_pages, k_scale, v_scale, block_table, lens):
    """fp64 (O [B,Hq,D], LSE [B,Hq]) of fa2_decode_paged_fp8: paged_decode_reference.ref_decode_paged on the pools dequantised to fp32."""
    kp = dequantize(k_pages.cpu(), per_head(k_scale.cpu()))
    vp = dequantize(v_pages.cpu(), per_head(v_scale.cpu()))
    return pr.ref_decode_paged(q, kp, vp, block_table, lens)


def make_pool(k8, v8, page, lens, order="shuffle", seed=0, extra=0):
    """paged_decode_reference.make_pool for dense e4m3fn caches k8, v8 [B,Hkv,Nmax,D]: every page no live entry names -- the poison page among
    them -- holds the NaN byte 0x7f. Returns (k_pages, v_pages e4m3fn, block_table int32 [B,max_pages])."""
    kp, vp, bt = pr.make_pool(bits(k8), bits(v8), page, lens, order=order, seed=seed, extra=extra, fill=NAN_BYTE)
    return kp.view(F8), vp.view(F8), bt
