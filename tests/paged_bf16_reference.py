"""Helpers of the bf16 paged KV-cache tests (tests/test_paged_bf16_surface.py, tests/test_gpu_paged_bf16_attention.py,
tests/test_gpu_paged_bf16_step.py): Python mirrors of the three bf16 describe texts, and the EMULATION the tolerance of O is measured against. The
fp64 references are the existing ones (prefill_varlen_reference.ref_prefill_paged_varlen, multi_decode_reference.ref_decode_paged_multi), which
convert their inputs to double and so take bf16 tensors as they are.

The bound of O is not a fixed number. For a case with the fp64 reference O_64,
    max|O - O_64| <= 2 max|O_emul - O_64| + 2^-8 max|O_64|,
where O_emul follows the kernel's roundings on the CPU (emul_rows below): scores from the bf16 inputs in fp64, cast to fp32; P = exp2 of the
scaled scores minus the row's FINAL maximum; P rounded to bf16; P V accumulated in fp64; divided by the fp32 row sum of the unrounded P; O rounded
to bf16. The second term is one half-ulp of the bf16 output store, the factor 2 covers the online rescaling order the emulation does not model.
LSE is fp32 and keeps decode_reference.lse_tol.

Largest err / bound of O seen on an MI355X over every case of tests/test_gpu_paged_bf16_attention.py and tests/test_gpu_paged_bf16_step.py: 0.323
(multi decode split over the keys, D = 64, lengths [4096, 1024, 257, 100, 0]); prefill 0.313 (D = 64, case 1x8x64x8, context 64); with V scaled
by 2^17 and K by 2^4 0.277 (prefill) and 0.278 (multi); the captured steps 0.302. No case exceeds 0.8. LSE: at most 0.0002 of lse_tol.

A plain module: nothing here is collected."""
import torch

import multi_decode_reference as mr
import paged_decode_reference as pr
import prefill_reference as pf
import prefill_varlen_reference as vr

ROW_TILE, KEY_STEP = vr.ROW_TILE, vr.KEY_STEP
LOG2E = 1.4426950408889634


def describe_prefill_text(B, total_q, Hq, Hkv, max_pages, page, D):
    """The text of cln_fa2_prefill_paged_varlen_bf16_describe: the fp16 text with the kernel's name and the bf16 MFMA."""
    text = vr.describe_prefill_text(B, total_q, Hq, Hkv, max_pages, page, D)
    assert text.count("fa2_prefill_paged_varlen_mfma<") == 1 and text.count("v_mfma_f32_16x16x32_f16") == 1
    return text.replace("fa2_prefill_paged_varlen_mfma<", "fa2_prefill_paged_varlen_bf16_mfma<").replace("16x16x32_f16", "16x16x32_bf16")


def describe_append_text(B, total_q, Hq, Hkv, max_pages, page, D, mode):
    """The text of cln_kv_append_paged_varlen_bf16_describe: the fp16 text with the kernel's name."""
    text = vr.describe_append_text(B, total_q, Hq, Hkv, max_pages, page, D, mode)
    assert text.count("kv_append_paged_varlen_rows<") == 1
    return text.replace("kv_append_paged_varlen_rows<", "kv_append_paged_varlen_bf16_rows<")


def describe_multi_text(B, T, Hq, Hkv, max_pages, page, D):
    """The text of cln_fa2_decode_paged_multi_bf16_describe, written out (the fp16 text has no Python mirror to derive it from)."""
    G = Hq // Hkv
    tiles = -(-T * G // mr.TILE_ROWS)
    S, C, ws = mr.plan(B, T, Hq, Hkv, max_pages, page, D)
    text = ("fa2_decode_paged_multi_bf16_mfma<D=%d,MT=%d> T=%d G=%d S=%d C=%d page=%d: 4 waves split the %d-key steps, K rows through the block "
            "table straight to MFMA fragments, V rows through a transposed LDS read, each row loaded once for the %d query rows (T x G, "
            "%d tiles of 16) of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, fp32 scores, causal mask by "
            "select, online softmax" % (D, tiles, T, G, S, C, page, mr.KEY_STEP, T * G, tiles))
    if S > 1:
        text += ("; then fa2_decode_combine_bf16_rows<D=%d> merges the live splits of a query row by log-sum-exp in ascending order (workspace %d bytes)"
                 % (D, ws))
    return text + "; deterministic"


def emul_rows(q, k, v, vis):
    """O_emul, fp64 [R,D] holding bf16 values: queries q [R,D] over keys k, v [N,D] (bf16), query r seeing the first vis[r] keys; vis[r] = 0 gives a
    zero row. The six steps of the module's docstring."""
    R, D = q.shape
    out = torch.zeros(R, D, dtype=torch.float64)
    top = int(max(vis)) if len(vis) else 0
    if top == 0:
        return out
    vist = torch.tensor(list(vis), dtype=torch.int64)
    live = vist > 0
    s = (q.double() @ k[:top].double().T).float() * torch.tensor(LOG2E / D ** 0.5, dtype=torch.float32)  # 1: fp64 scores, cast to fp32, scaled there
    s = s.masked_fill(torch.arange(top)[None, :] >= vist[:, None], float("-inf"))[live]
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)                                                # 2: fp32, the row's final maximum
    lsum = p.sum(dim=-1, dtype=torch.float32)                                                              # 5: fp32 row sum of the unrounded P
    o = p.bfloat16().double() @ v[:top].double()                                                           # 3, 4
    out[live] = (o / lsum.double()[:, None]).float().bfloat16().double()                                   # 5, 6
    return out


def _emul_sequence(qb, kd, vd, vis_t):
    """O_emul [T,Hq,D] of one sequence: qb bf16 [T,Hq,D], kd / vd its gathered dense cache [Hkv,N,D], vis_t [T]."""
    T, Hq, D = qb.shape
    G = Hq // kd.shape[0]
    out = torch.zeros(T, Hq, D, dtype=torch.float64)
    for h in range(Hq):
        out[:, h] = emul_rows(qb[:, h], kd[h // G], vd[h // G], vis_t)
    return out


def emul_prefill_paged_varlen(q, k_pages, v_pages, block_table, lens, cu):
    """O_emul [total_q,Hq,D] of the packed q; NaN in the rows of no sequence, as the reference has them."""
    Nmax = block_table.shape[1] * k_pages.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (k_pages, v_pages))
    out = torch.full(q.shape, float("nan"), dtype=torch.float64)
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        if hi > lo:
            out[lo:hi] = _emul_sequence(q[lo:hi], k[b], v[b], pf.visible([lens[b]], hi - lo, Nmax)[0].tolist())
    return out


def emul_decode_paged_multi(q, k_pages, v_pages, block_table, lens):
    """O_emul [B,T,Hq,D]."""
    B, T = q.shape[:2]
    Nmax = block_table.shape[1] * k_pages.shape[2]
    k, v = (pr.gather(t, block_table, lens) for t in (k_pages, v_pages))
    vis = mr.visible(lens, T, Nmax)
    return torch.stack([_emul_sequence(q[b], k[b], v[b], vis[b * T:(b + 1) * T]) for b in range(B)])


def o_bound(o_emul, o_ref):
    """2 max|O_emul - O_64| + 2^-8 max|O_64| over the rows of the sequences (the finite entries of the reference)."""
    fin = torch.isfinite(o_ref)
    return 2.0 * float((o_emul[fin] - o_ref[fin]).abs().max()) + 2.0 ** -8 * float(o_ref[fin].abs().max())
