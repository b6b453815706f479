"""References for the tests of the two MFMA attention entries over an FP8 (e4m3fn) paged KV cache, fa2_prefill_paged_fp8 and
fa2_decode_paged_multi_fp8 (tests/test_fa2_prefill_paged_fp8_surface.py and tests/test_fa2_decode_paged_multi_fp8_surface.py prove them on the
CPU; tests/test_gpu_fa2_prefill_paged_fp8.py and tests/test_gpu_fa2_decode_paged_multi_fp8.py use them through tests/fp8_paged_attn_cases.py):
the unmodified fp64 references of prefill_reference / multi_decode_reference on pools dequantised with fp8_kv_reference.dequantize, and Python
mirrors of the plan of csrc/flash_attn_decode_paged_multi_fp8.hip and of the two describe texts. A plain module: nothing here is collected."""
import decode_reference as dr
import fp8_kv_reference as f8
import multi_decode_reference as mr
import prefill_reference as pf

KEY_STEP = 128  # keys per workgroup step of fa2pm::fa2_decode_paged_multi_fp8_mfma: 4 waves x 32 keys, for both head dims (the fp16 kernel's)
ROW_TILE, PREFILL_KEY_STEP = pf.ROW_TILE, pf.KEY_STEP  # the tile of fa2pp::fa2_prefill_paged_fp8_mfma is the fp16 kernel's


def _dequantised(k_pages, v_pages, k_scale, v_scale):
    return f8.dequantize(k_pages.cpu(), f8.per_head(k_scale.cpu())), f8.dequantize(v_pages.cpu(), f8.per_head(v_scale.cpu()))


def ref_prefill_paged_fp8(q, k_pages, v_pages, k_scale, v_scale, block_table, lens):
    """fp64 (O [B,T,Hq,D], LSE [B,T,Hq]) of fa2_prefill_paged_fp8: prefill_reference.ref_prefill_paged on the pools dequantised to fp32."""
    kp, vp = _dequantised(k_pages, v_pages, k_scale, v_scale)
    return pf.ref_prefill_paged(q, kp, vp, block_table, lens)


def ref_decode_paged_multi_fp8(q, k_pages, v_pages, k_scale, v_scale, block_table, lens):
    """fp64 (O [B,T,Hq,D], LSE [B,T,Hq]) of fa2_decode_paged_multi_fp8: multi_decode_reference.ref_decode_paged_multi on the pools dequantised
    to fp32."""
    kp, vp = _dequantised(k_pages, v_pages, k_scale, v_scale)
    return mr.ref_decode_paged_multi(q, kp, vp, block_table, lens)


def plan(B, T, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) as cln_fa2_decode_paged_multi_fp8_plan computes them: B Hkv workgroups per split whatever T is, the
    chunk a multiple of max(page, KEY_STEP), the three constants of decode_reference."""
    Nmax, unit, bk = max_pages * page, max(page, KEY_STEP), B * Hkv
    want = 1
    if bk < dr.TARGET_WORKGROUPS and Nmax > dr.MIN_CHUNK:
        want = min(-(-dr.TARGET_WORKGROUPS // bk), Nmax // dr.MIN_CHUNK, dr.MAX_SPLITS)
    chunk = -(-(-(-Nmax // want)) // unit) * unit
    splits = -(-Nmax // chunk)
    return splits, chunk, (B * T * Hq * splits * (D + 2) * 4 if splits > 1 else 0)


def describe_multi_text(B, T, Hq, Hkv, max_pages, page, D):
    """The text of cln_fa2_decode_paged_multi_fp8_describe for a supported shape."""
    G = Hq // Hkv
    S, C, need = plan(B, T, Hq, Hkv, max_pages, page, D)
    tiles = -(-T * G // 16)
    t = ("fa2_decode_paged_multi_fp8<D=%d,MT=%d> T=%d G=%d S=%d C=%d page=%d: 4 waves split the %d-key steps, e4m3 K and V rows "
         "through the block table to registers, 16 bytes per lane, converted to fp16 once (v_cvt_scalef32_pk_f16_fp8, exact): K "
         "to MFMA fragments, V through a transposed LDS read, each row loaded once for the %d query rows (T x G, %d tiles of 16) "
         "of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16, fp32 scores times k_scale, causal mask by "
         "select, online softmax, the partial times v_scale" % (D, tiles, T, G, S, C, page, KEY_STEP, T * G, tiles))
    if S > 1:
        t += ("; then fa2_decode_combine<D=%d> merges the live splits of a query row by log-sum-exp in ascending order (workspace %d bytes)"
              % (D, need))
    return t + "; deterministic"


def describe_prefill_text(B, T, Hq, Hkv, max_pages, page, D):
    """The text of cln_fa2_prefill_paged_fp8_describe for a supported shape."""
    G = Hq // Hkv
    nt = pf.tiles(T, G)
    return ("fa2_prefill_paged_fp8<D=%d,G=%d> T=%d page=%d rows=%d keys=%d: one launch, no workspace; %d workgroups of 256 threads "
            "(%d (sequence, KV head) pairs x %d tiles of %d of the %d query rows t G + g, 32 rows per wave), each walks the keys "
            "below the causal edge of its last token in steps of %d, e4m3 K and V rows through the block table, 8 bytes per thread "
            "and row, converted to fp16 once on their way to LDS (v_cvt_scalef32_pk_f16_fp8, exact), S^T = K Q^T and O^T = V^T P^T on "
            "v_mfma_f32_16x16x32_f16, V through ds_read_b64_tr_b16, fp32 scores times k_scale, causal mask by select on the steps that "
            "cross the edge, online softmax, the normalisation times v_scale, no split over the keys; deterministic"
            % (D, G, T, page, ROW_TILE, PREFILL_KEY_STEP, B * Hkv * nt, B * Hkv, nt, ROW_TILE, T * G, PREFILL_KEY_STEP))
