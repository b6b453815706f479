"""Helpers of the tests of the bf16 paged entries over FP8 (e4m3) pools (tests/test_paged_bf16_fp8_surface.py,
tests/test_gpu_paged_bf16_fp8_attention.py, tests/test_gpu_kv_append_paged_varlen_bf16_fp8.py): the per-head scales, the quantised forms of the
cases of paged_sink_reference, the fp64 reference and the bf16 emulation ON THE DEQUANTISED POOLS, the append on the CPU, and mirrors of the three
describe texts.

No new tolerance. A stored byte c of KV head h means e4m3(c) * scale[h]; fp8_kv_reference.dequantize(..., torch.float64) is exact, and
O_64 / LSE_64 / O_emul are paged_sink_reference.prefill / .decode on those float64 pools (sinks = None: a sink of -inf per head). O is held to
paged_bf16_reference.o_bound(O_emul, O_64), LSE to decode_reference.lse_tol per head, -inf rows and zero rows exactly. The kernels differ from
the emulation only in where the two scale products round in fp32 -- (q . code) * (k_scale log2(e) / sqrt(D)) against (q . (code k_scale)) *
(log2(e) / sqrt(D)), and acc * (v_scale / l) against (P (code v_scale)) / l -- a few 2^-24 relative, which the bound's factor 2 is there for.

The scales differ by at least a factor 2 between neighbouring KV heads, so that a kernel that reads another head's scale, or drops one, is more
than 4 x the bound away (shown on the CPU by the surface test, on every case the GPU file runs with these scales).

Largest err / bound of O seen on an MI355X over every case of tests/test_gpu_paged_bf16_fp8_attention.py (profiles/r23_paged_bf16_fp8_tests.log):
prefill 0.334 (D = 64, 1 x 1 heads, page 64, no window, mixed sinks), decode with one split 0.314 (D = 64, T = 3, G = 8, W = 33, mixed sinks),
with several splits 0.328 (D = 64, G = 1, no window, len 4096, no sinks), the gpt-oss chain append -> prefill -> decode 0.281, all 254 finite
codes in K and V 0.312. No case exceeds 0.4. LSE: at most 0.0002 of lse_tol (0.066 on the gpt-oss chain, whose reference rotates q on the
CPU). The append's rotated K rows: at most 0.996 of fp8_kv_reference.bound (the e4m3 half-ulp itself), q_out within kv_append_bf16_reference.bound.

A plain module: nothing here is collected."""
import torch

import fp8_kv_reference as f8
import kv_append_bf16_reference as ar
import kv_append_reference as kr
import paged_sink_reference as sr
import paged_window_reference as wr

BF = torch.bfloat16
NEG_INF = float("-inf")
NAN_BYTE = f8.NAN_BYTE
FINITE_CODES = [c for c in range(256) if c & 0x7F != 0x7F]


def scales(Hkv, pow2=False):
    """(k_scale, v_scale) fp32 [Hkv]: neighbours differ by a factor >= 2; pow2: powers of two only (the dequantised pools are then bf16 tensors)."""
    kb = [1.0, 4.0, 0.5, 2.0] if pow2 else [1.0, 2.5, 0.5, 1.75, 0.75, 3.0, 1.25, 0.375]
    vb = [2.0, 0.5, 4.0, 1.0] if pow2 else [1.5, 0.5, 2.25, 0.875, 3.5, 1.0, 0.4375, 2.0]
    ks = torch.tensor([2.0 ** -3 * kb[h % len(kb)] for h in range(Hkv)], dtype=torch.float32)
    vs = torch.tensor([2.0 ** -2 * vb[h % len(vb)] for h in range(Hkv)], dtype=torch.float32)
    return ks, vs


def quantize_pool(pages, scale):
    """e4m3 pool of a bf16 pool [P,Hkv,page,D] (paged_decode_reference.make_pool: NaN in every page no live entry names) under scale [Hkv]; the NaN
    elements become the byte 0x7F."""
    nan = torch.isnan(pages.float())
    c = f8.bits(f8.quantize(torch.where(nan, torch.zeros_like(pages), pages), f8.per_head(scale))).clone()
    c[nan] = NAN_BYTE
    return c.view(f8.F8)


def quantize_pools(pool, ks, vs):
    kp, vp, bt = pool
    return quantize_pool(kp, ks), quantize_pool(vp, vs), bt


def dq(pages8, scale):
    """The float64 pool the reference runs on: exact."""
    return f8.dequantize(pages8, f8.per_head(scale), torch.float64)


def _sinks(sinks, Hq):
    return torch.full((Hq,), NEG_INF, dtype=torch.float32) if sinks is None else sinks


def prefill(q, kp8, vp8, bt, lens, cu, ks, vs, W, sinks, count=1):
    """(O_64, LSE_64, O_emul) of the packed q over the e4m3 pools; NaN in the rows of no sequence."""
    return sr.prefill(q, dq(kp8, ks), dq(vp8, vs), bt, lens, cu, W, _sinks(sinks, q.shape[-2]), count)


def decode(q, kp8, vp8, bt, lens, ks, vs, W, sinks, count=1):
    return sr.decode(q, dq(kp8, ks), dq(vp8, vs), bt, lens, W, _sinks(sinks, q.shape[-2]), count)


def wrong_scales(ks, vs):
    """The mistakes a kernel can make with the scales: k_scale dropped, v_scale dropped, the neighbouring head's scales (only with Hkv > 1)."""
    one = torch.ones_like(ks)
    out = [("no k_scale", one, vs), ("no v_scale", ks, one)]
    if ks.numel() > 1:
        out.append(("neighbour's scales", ks.roll(1), vs.roll(1)))
    return out


# ---------------------------------------------------------------------------------------------------- the cases both test files look at

PREFILL_WINDOWS = [1, 65, None]


def prefill_case(D, Hq, Hkv, page):
    """paged_sink_reference.prefill_case with its pools quantised: (qs, lens, (kp8, vp8, bt), ks, vs)."""
    qs, lens, pool = sr.prefill_case(D, Hq, Hkv, page)
    ks, vs = scales(Hkv)
    return qs, lens, quantize_pools(pool, ks, vs), ks, vs


def decode_one_case(T, G, D):
    q, lens, pool = sr.decode_one_case(T, G, D)
    ks, vs = scales(sr.ONE_HKV)
    return q, lens, quantize_pools(pool, ks, vs), ks, vs


SPLIT_LENS = [4096, 257]
SPLIT_G = [1, 8]


def decode_split_case(G, D, n):
    """T = 1, Hkv = 1, Nmax 16384."""
    q, lens, pool = sr.decode_split_case(1, G, D, n)
    ks, vs = scales(1)
    return q, lens, quantize_pools(pool, ks, vs), ks, vs


def all_codes_case(D):
    """A dense cache [1,1,512,D] whose K and V rows run through all 254 finite e4m3 codes (subnormals included, every code in K and in V), scale
    1, in pages of 16; queries randn / 64 (the codes reach 448: the scores stay of order one)."""
    N = 512
    codes = torch.tensor(FINITE_CODES, dtype=torch.uint8)
    idx = torch.arange(N * D)
    k8 = codes[(idx * 37 + idx // D) % 254].view(1, 1, N, D)
    v8 = codes[(idx * 101 + 7 * (idx // D) + 3) % 254].view(1, 1, N, D)
    assert set(k8.flatten().tolist()) == set(FINITE_CODES) == set(v8.flatten().tolist())
    one = torch.ones(1, dtype=torch.float32)
    return k8.view(f8.F8), v8.view(f8.F8), one, one, N


# ---------------------------------------------------------------------------------------------------- append

def ref_append(k_new, v_new, kp8, vp8, bt, lens, cu, ks, vs, q, table, mode):
    """cln_kv_append_paged_varlen_bf16_fp8 on the CPU: kv_append_bf16_reference.ref_append_varlen decides liveness and rotates (fp64), the bytes are
    fp8_kv_reference.quantize of the bf16 input (V, and K without a rotation: byte for byte) or of the fp64 rotation rounded to fp32 (compare
    those through rows and fp8_kv_reference.bound). Returns (k bytes, v bytes, k_live, rows, dead) as there, the pools as uint8."""
    P, Hkv, page, D = kp8.shape
    blank = torch.zeros(P, Hkv, page, D, dtype=BF)
    _, _, k_live, rows, dead = ar.ref_append_varlen(k_new, v_new, blank, blank, bt, lens, cu, q, table, mode)
    kb, vb = f8.bits(kp8).clone(), f8.bits(vp8).clone()
    for (row, b, pos, k_rot, _, _, _) in rows:
        pg, r = int(bt[b, pos // page]), pos % page
        kb[pg, :, r] = f8.bits(f8.quantize(k_new[row] if mode == 0 else k_rot.float(), ks.reshape(-1, 1)))
        vb[pg, :, r] = f8.bits(f8.quantize(v_new[row], vs.reshape(-1, 1)))
    return kb, vb, k_live, rows, dead


# ---------------------------------------------------------------------------------------------------- describe texts

def describe_prefill_text(B, total_q, Hq, Hkv, max_pages, page, D, W):
    """The text of cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8_describe, derived from the sink entry's."""
    text = sr.describe_prefill_text(B, total_q, Hq, Hkv, max_pages, page, D, W)
    for old, new in (("fa2_prefill_paged_varlen_window_sink_bf16_mfma<", "fa2_prefill_paged_varlen_window_sink_bf16_fp8_mfma<"),
                     ("whatever the length; K and V rows through the block table to LDS once per workgroup,",
                      "whatever the length; e4m3 K and V rows through the block table, 8 bytes per thread and row, converted to bf16 once on their "
                      "way to LDS (v_cvt_scalef32_pk_bf16_fp8, exact), once per workgroup,"),
                     ("fp32 scores, window", "fp32 scores times k_scale, window"),
                     ("online softmax, no split", "online softmax, the normalisation times v_scale, no split"),
                     ("natural log, unscaled)", "natural log, unscaled; none when sinks is NULL)")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    return text


def describe_multi_text(B, T, Hq, Hkv, max_pages, page, D, W):
    """The text of cln_fa2_decode_paged_multi_window_sink_bf16_fp8_describe, derived from the sink entry's."""
    text = sr.describe_multi_text(B, T, Hq, Hkv, max_pages, page, D, W)
    split = wr.plan(B, T, Hq, Hkv, max_pages, page, D, W)[0] > 1
    subs = [("fa2_decode_paged_multi_window_sink_bf16_mfma<", "fa2_decode_paged_multi_window_sink_bf16_fp8_mfma<"),
            ("-key steps, K rows through the block table straight to MFMA fragments, V rows through a transposed LDS read,",
             "-key steps, e4m3 K and V rows through the block table to registers, 16 bytes per lane, converted to bf16 once "
             "(v_cvt_scalef32_pk_bf16_fp8, exact): K to MFMA fragments, V through a transposed LDS read,"),
            ("fp32 scores, window", "fp32 scores times k_scale, window"),
            ("online softmax;", "online softmax, the partial times v_scale;")]
    if split:
        subs.append(("natural log, unscaled)", "natural log, unscaled; none when sinks is NULL: fa2_decode_combine_window_bf16_rows<D=%d> then)" % D))
    else:
        subs.append(("natural log, unscaled)", "natural log, unscaled; none when sinks is NULL)"))
    for old, new in subs:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    return text


ROT = ["rows not rotated", "K and q rotated in half-split pairs (i, i + D/2)", "K and q rotated in interleaved pairs (2i, 2i + 1)"]


def describe_append_text(B, total_q, Hq, Hkv, max_pages, page, D, mode):
    """The text of cln_kv_append_paged_varlen_bf16_fp8_describe, written out: the workgroups per packed row are those of the bf16 entry (a thread
    per 8 elements; with the half-split rotation per 16)."""
    rows = 2 * Hkv + (Hq if mode else 0)
    y = -(-rows * (D // 16 if mode == 1 else D // 8) // 256)
    return ("kv_append_paged_varlen_bf16_fp8_rows<D=%d,ROPE=%d> B=%d total_q=%d page=%d: one launch, no workspace; %d x %d workgroups of 256 threads "
            "(a packed row x the 8-element pieces of its %d K, %d V and %d q rows), the sequence of a row by binary search over the device-side "
            "offsets, length and table entry through uniform loads, %s%s, K and V times 1 / scale of their KV head in fp32, clamped to +-448 and "
            "rounded to nearest even to e4m3, 8-byte plain stores into the pools; deterministic"
            % (D, mode, B, total_q, page, total_q, y, Hkv, Hkv, Hq if mode else 0, ROT[mode],
               " in fp32 from the cos/sin table, q rounded once to bf16 at the store" if mode else ""))
