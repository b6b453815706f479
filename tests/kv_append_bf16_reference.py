"""Reference for the bf16 paged KV-cache append tests (tests/test_gpu_paged_bf16_step.py): cuda_learn_notes_amd.kv_append_paged_varlen_bf16 /
cln_kv_append_paged_varlen_bf16 (csrc/kv_append_paged_varlen_bf16.cuh) on the CPU. kv_append_reference rounds its pool rows to fp16, so the
packed loop is written out here for bf16; the rotation itself is the unmodified kv_append_reference.rotate (fp64 from the inputs' exact values
and the fp32 table values). The bound is derived, not measured. A plain module: nothing here is collected."""
import torch

import kv_append_reference as kr


def bound(r, mag):
    """kv_append_reference.bound with the half-ulp of bf16 and no subnormal floor (bf16 has the exponent range of fp32: no test value comes near
    its subnormals):
        2^-8 |r|      the one rounding to bf16, round to nearest even: half an ulp of 2^-7 relative,
      + 2^-22 mag     the fp32 arithmetic in front of it, as there: at most three roundings of 2^-24 relative each, and the double rounding
                      fp64 -> fp32 -> bf16. bf16 inputs and fp32 table values are exact in fp32."""
    return 2.0 ** -8 * r.abs() + 2.0 ** -22 * mag


def ref_append_varlen(k_new, v_new, k_pages, v_pages, block_table, lens, cu, q, table, mode):
    """The call on the CPU: packed k_new, v_new bf16 [total_q,Hkv,D], pools bf16 [P,Hkv,page,D] (copied, not modified), lens B Python ints, cu the
    B + 1 offsets, q bf16 [total_q,Hq,D] or None, table fp32 [max_pos,D] or None, mode 0 / 1 / 2. Token i of sequence b is packed row cu[b] + i at
    pos = lens[b] - T_b + i, live iff 0 <= pos < max_pages page (and pos < max_pos with a rotation). Returns (k_pages, v_pages, k_live bool
    [P,page], rows, dead): the pools after the call (a rotated K row holds the fp64 value rounded once to bf16 -- compare those through rows and
    bound()), the pool rows the call writes, rows = (packed row, b, pos, k_rot, k_mag, q_rot, q_mag) of every LIVE token (fp64; the last two None
    without q) and dead = the packed rows of the sequences' tokens that are not live."""
    P, _, page, _ = k_pages.shape
    cap = block_table.shape[1] * page
    kp, vp = k_pages.clone(), v_pages.clone()
    k_live = torch.zeros(P, page, dtype=torch.bool)
    rows, dead = [], []
    for b in range(len(cu) - 1):
        T = cu[b + 1] - cu[b]
        for i in range(T):
            row, pos = cu[b] + i, int(lens[b]) - T + i
            if not (0 <= pos < cap) or (mode != 0 and pos >= table.shape[0]):
                dead.append(row)
                continue
            pg, r = int(block_table[b, pos // page]), pos % page
            assert 0 <= pg < P and not bool(k_live[pg, r]), "the caller's contract: live entries in [0, P), no page named twice"
            k_live[pg, r] = True
            trow = table[pos] if mode != 0 else None
            k_rot, k_mag = kr.rotate(k_new[row], trow, mode)
            kp[pg, :, r] = k_new[row] if mode == 0 else k_rot.float().bfloat16()
            vp[pg, :, r] = v_new[row]
            q_rot = q_mag = None
            if q is not None:
                q_rot, q_mag = kr.rotate(q[row], trow, mode)
            rows.append((row, b, pos, k_rot, k_mag, q_rot, q_mag))
    return kp, vp, k_live, rows, dead
