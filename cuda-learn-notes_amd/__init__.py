"""cuda-learn-notes_amd: MI355X (gfx950) native drop-in for the HGEMM / FlashAttention-2 hot path
of DefTruth/CUDA-Learn-Notes and its supporting reduce/softmax/layer-norm/rms-norm/rope/elementwise
kernels. Host code is Python on PyTorch-ROCm calling hand-written HIP kernels through a C-ABI
(see include/cln_amd.h)."""
from . import manifest  # noqa: F401


def build(verbose=False, force=False):
    from . import _build
    return _build.build(verbose=verbose, force=force)


def load(*groups):
    """`lib = load('elementwise')` ~ reference `lib = load(name='elementwise_lib', sources=[...])`."""
    from . import host
    return host.load_lib(*groups)


def hgemm_lib():
    """Mirror of `import toy_hgemm` / try_load_hgemm_library (kernels/hgemm/tools/utils.py:116-132)."""
    return load("hgemm", "hgemm_vendor", "hgemm_vendor_lt")


def flash_attn_lib():
    return load("flash_attn")


def fa2_fwd_causal(Q, K, V, O, stages=2):
    """Causal FlashAttention-2 forward (mask key <= query) into O; fp16 [B,H,N,D], D in {64, 128}, N % 256 == 0.
    C entry: cln_fa2_fwd_causal (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_fwd_causal(Q, K, V, O, stages)


def fa2_fwd_lse(Q, K, V, O, LSE, causal=False, stages=2):
    """FlashAttention-2 forward into O that also writes the row log-sum-exp LSE (fp32 [B,H,N], natural log); fp16 [B,H,N,D],
    D in {64, 128}, N % 256 == 0. C entries cln_fa2_fwd_lse / cln_fa2_fwd_causal_lse (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_fwd_lse(Q, K, V, O, LSE, causal, stages)


def fa2_bwd(Q, K, V, O, dO, LSE, dQ, dK, dV, delta=None, causal=False):
    """FlashAttention-2 backward into dQ, dK, dV from the forward's O and LSE (fa2_fwd_lse); deterministic. C entries cln_fa2_bwd /
    cln_fa2_bwd_causal (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_bwd(Q, K, V, O, dO, LSE, dQ, dK, dV, delta, causal)


def fa2_decode(q, k_cache, v_cache, seqlens, out, lse=None, workspace=None):
    """Single-query (decode) attention over a KV cache into out: q, out fp16 [B,H,D], caches fp16 [B,H,Nmax,D], seqlens int32 [B] on the GPU,
    lse fp32 [B,H] or None; D in {64, 128}, any Nmax. C entry cln_fa2_decode (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode(q, k_cache, v_cache, seqlens, out, lse, workspace)


def fa2_decode_plan(B, H, Nmax, D):
    """(splits, chunk, workspace_bytes) of fa2_decode for this shape; depends on nothing else. C entry cln_fa2_decode_plan."""
    from . import host
    return host.fa2_decode_plan(B, H, Nmax, D)


def fa2_decode_paged(q, k_pages, v_pages, block_table, seqlens, out, lse=None, workspace=None):
    """Decode attention over a paged KV cache with grouped query heads into out: q, out fp16 [B,Hq,D], k_pages / v_pages fp16 [P,Hkv,page,D],
    block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU, lse fp32 [B,Hq] or None; D in {64, 128}, Hq / Hkv in {1, 2, 4, 8}, page in
    {16, ..., 256}. C entry cln_fa2_decode_paged (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged(q, k_pages, v_pages, block_table, seqlens, out, lse, workspace)


def fa2_decode_paged_plan(B, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged for this shape; depends on nothing else. C entry cln_fa2_decode_paged_plan."""
    from . import host
    return host.fa2_decode_paged_plan(B, Hq, Hkv, max_pages, page, D)


def fa2_decode_paged_multi(q, k_pages, v_pages, block_table, seqlens, out, lse=None, workspace=None):
    """Multi-token decode attention (speculative verify, short appends) over a paged KV cache with grouped query heads into out: q, out fp16
    [B,T,Hq,D], k_pages / v_pages fp16 [P,Hkv,page,D], block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (the lengths count the T
    newest tokens), lse fp32 [B,T,Hq] or None; query t sees the keys j < len - (T - 1 - t). T in 1 … 8, D in {64, 128}, Hq / Hkv in
    {1, 2, 4, 8}, page in {16, ..., 256}. C entry cln_fa2_decode_paged_multi (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi(q, k_pages, v_pages, block_table, seqlens, out, lse, workspace)


def fa2_decode_paged_multi_plan(B, T, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi for this shape; depends on nothing else. C entry
    cln_fa2_decode_paged_multi_plan."""
    from . import host
    return host.fa2_decode_paged_multi_plan(B, T, Hq, Hkv, max_pages, page, D)


def kv_append_paged(k_new, v_new, k_pages, v_pages, block_table, seqlens, q=None, q_out=None, rope_table=None, rope="none"):
    """Write the K / V rows of T new tokens per sequence into a paged KV cache (the pools, table and lengths of fa2_decode_paged_multi; the
    lengths count the new tokens), with the rotary embedding of K and q fused in: k_new, v_new fp16 [B,T,Hkv,D], q / q_out fp16 [B,T,Hq,D] or
    None (q_out may be q), rope_table fp32 [max_pos,D] (kv_append_rope_table), rope "none", "half" (pairs (i, i + D/2)) or "interleaved"
    (pairs (2i, 2i+1)). One launch, nothing read on the host. C entry cln_kv_append_paged (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.kv_append_paged(k_new, v_new, k_pages, v_pages, block_table, seqlens, q, q_out, rope_table, rope)


def kv_append_rope_table(max_pos, D, theta=10000.0, device=None):
    """fp32 [max_pos, D] for kv_append_paged: row p = cos(p f_i) for i < D/2, then sin(p f_i), f_i = theta^(-2i/D), angles formed in float64."""
    from . import host
    return host.kv_append_rope_table(max_pos, D, theta, device)


def fa2_prefill_paged(q, k_pages, v_pages, block_table, seqlens, out, lse=None):
    """Prefill attention (a prompt or a chunk of one, any T >= 1) over a paged KV cache with grouped query heads into out: the tensors and the
    semantics of fa2_decode_paged_multi with T unbounded -- the lengths count the T newest tokens, query t sees the keys
    j < len - (T - 1 - t), a sequence with len < T has its live tokens right-aligned as kv_append_paged writes them. One launch, no workspace.
    D in {64, 128}, Hq / Hkv in {1, 2, 4, 8}, page in {16, ..., 256}. C entry cln_fa2_prefill_paged (include/cln_amd_ext.h). Not a reference
    name."""
    from . import host
    return host.fa2_prefill_paged(q, k_pages, v_pages, block_table, seqlens, out, lse)


def kv_append_paged_fp8(k_new, v_new, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged into an FP8 cache: k_pages / v_pages torch.float8_e4m3fn [P,Hkv,page,D], k_scale / v_scale fp32 [Hkv] on the GPU (a stored
    byte c of KV head h means e4m3(c) * scale[h]); K and V are multiplied by 1 / scale in fp32, clamped to +-448 and rounded to nearest even, q is
    rotated and written as fp16 without a scale. Everything else as kv_append_paged. C entry cln_kv_append_paged_fp8 (include/cln_amd_ext.h).
    Not a reference name."""
    from . import host
    return host.kv_append_paged_fp8(k_new, v_new, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, q, q_out, rope_table, rope)


def fa2_decode_paged_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse=None, workspace=None):
    """fa2_decode_paged over an FP8 cache: k_pages / v_pages torch.float8_e4m3fn [P,Hkv,page,D], k_scale / v_scale fp32 [Hkv] on the GPU; q, out
    fp16 [B,Hq,D], lse fp32 [B,Hq] or None. Everything else as fa2_decode_paged. C entry cln_fa2_decode_paged_fp8 (include/cln_amd_ext.h). Not
    a reference name."""
    from . import host
    return host.fa2_decode_paged_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse, workspace)


def fa2_decode_paged_fp8_plan(B, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_fp8 for this shape; depends on nothing else. C entry cln_fa2_decode_paged_fp8_plan."""
    from . import host
    return host.fa2_decode_paged_fp8_plan(B, Hq, Hkv, max_pages, page, D)


def fa2_decode_paged_multi_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse=None, workspace=None):
    """fa2_decode_paged_multi over a paged KV cache held in FP8: k_pages, v_pages torch.float8_e4m3fn [P,Hkv,page,D], k_scale, v_scale fp32
    [Hkv] on the GPU; q, out fp16 [B,T,Hq,D], T in 1 … 8, lse fp32 [B,T,Hq] or None. Everything else as fa2_decode_paged_multi. C entry
    cln_fa2_decode_paged_multi_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse, workspace)


def fa2_decode_paged_multi_fp8_plan(B, T, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_fp8 for this shape; depends on nothing else. C entry
    cln_fa2_decode_paged_multi_fp8_plan."""
    from . import host
    return host.fa2_decode_paged_multi_fp8_plan(B, T, Hq, Hkv, max_pages, page, D)


def fa2_prefill_paged_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse=None):
    """fa2_prefill_paged over a paged KV cache held in FP8: k_pages, v_pages torch.float8_e4m3fn [P,Hkv,page,D], k_scale, v_scale fp32 [Hkv] on
    the GPU; q, out fp16 [B,T,Hq,D], any T >= 1, lse fp32 [B,T,Hq] or None. Everything else as fa2_prefill_paged. C entry
    cln_fa2_prefill_paged_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse)


def fa2_prefill_paged_varlen(q, k_pages, v_pages, block_table, seqlens, cu_q, out, lse=None):
    """fa2_prefill_paged for a packed batch with a per-sequence number of new tokens: q, out fp16 [total_q,Hq,D], lse fp32 [total_q,Hq] or None,
    cu_q int32 [B+1] on the GPU (never read by the host): the tokens of sequence b are the packed rows cu_q[b] .. cu_q[b+1]-1, T_b of them, and
    seqlens[b] counts them. Rows outside [cu_q[0], cu_q[B]) are not touched. A sequence's bits are those of fa2_prefill_paged on it alone. One
    launch, no workspace. C entry cln_fa2_prefill_paged_varlen (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen(q, k_pages, v_pages, block_table, seqlens, cu_q, out, lse)


def kv_append_paged_varlen(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged for a packed batch with a per-sequence number of new tokens: k_new, v_new fp16 [total_q,Hkv,D], q / q_out fp16
    [total_q,Hq,D] or None, cu_q int32 [B+1] on the GPU as for fa2_prefill_paged_varlen; token i of sequence b stands at
    seqlens[b] - T_b + i. Everything else as kv_append_paged. One launch, nothing read on the host. C entry cln_kv_append_paged_varlen
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.kv_append_paged_varlen(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q, q_out, rope_table, rope)


def kv_append_paged_varlen_bf16(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged_varlen on torch.bfloat16 tensors (new rows, q, q_out, pools; rope_table stays fp32): fp32 rotation from the bf16 inputs,
    one rounding to bf16, V and rope "none" rows copied bit for bit. Everything else as kv_append_paged_varlen; a fixed T is
    cu_q = T * arange(B + 1). C entry cln_kv_append_paged_varlen_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.kv_append_paged_varlen_bf16(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q, q_out, rope_table, rope)


def fa2_prefill_paged_varlen_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, out, lse=None):
    """fa2_prefill_paged_varlen on torch.bfloat16 tensors (q, out, pools; lse stays fp32): bf16 operands on the matrix cores, fp32 scores and
    accumulators, P and O rounded once to bf16, nothing through fp16. Everything else as fa2_prefill_paged_varlen. C entry
    cln_fa2_prefill_paged_varlen_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, out, lse)


def fa2_decode_paged_multi_bf16(q, k_pages, v_pages, block_table, seqlens, out, lse=None, workspace=None):
    """fa2_decode_paged_multi on torch.bfloat16 tensors (q, out [B,T,Hq,D], pools; lse and the workspace stay fp32), T in 1 … 8, split over the
    keys by fa2_decode_paged_multi_bf16_plan. Everything else as fa2_decode_paged_multi. C entry cln_fa2_decode_paged_multi_bf16
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_bf16(q, k_pages, v_pages, block_table, seqlens, out, lse, workspace)


def fa2_decode_paged_multi_bf16_plan(B, T, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_bf16: what fa2_decode_paged_multi_plan returns for the same numbers. C entry
    cln_fa2_decode_paged_multi_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_multi_bf16_plan(B, T, Hq, Hkv, max_pages, page, D)


def fa2_prefill_paged_varlen_window_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, out, lse=None):
    """fa2_prefill_paged_varlen_bf16 with a sliding window: the query at position p sees the keys max(0, p - window + 1) … p (HF
    sliding_window = window). Everything else as there; with window >= max_pages * page its bits. Pages wholly below the window of a sequence's
    first new token (aligned down to max(page, 64)) are not read, nor are their table entries. C entry
    cln_fa2_prefill_paged_varlen_window_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_window_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, out, lse)


def fa2_decode_paged_multi_window_bf16(q, k_pages, v_pages, block_table, seqlens, window, out, lse=None, workspace=None):
    """fa2_decode_paged_multi_bf16 with a sliding window (the mask of fa2_prefill_paged_varlen_window_bf16), T in 1 … 8, the window -- not
    max_pages * page -- split over the keys by fa2_decode_paged_multi_window_bf16_plan. Pages wholly below the window of the first query
    (aligned down to max(page, 128)) are not read, nor are their table entries. C entry cln_fa2_decode_paged_multi_window_bf16
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_window_bf16(q, k_pages, v_pages, block_table, seqlens, window, out, lse, workspace)


def fa2_decode_paged_multi_window_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_bf16; with window >= max_pages * page what
    fa2_decode_paged_multi_bf16_plan returns. C entry cln_fa2_decode_paged_multi_window_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_multi_window_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window)


def fa2_prefill_paged_varlen_window_sink_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, out, lse=None):
    """fa2_prefill_paged_varlen_window_bf16 with attention sinks: sinks fp32 [Hq] on the GPU, one logit per query head in natural-log units (not
    scaled by 1/sqrt(D)) that joins the softmax denominator of every row of its head and carries no value (HF GptOssAttention). lse is the log
    of that denominator, the sink included; a row that sees no key stays O = 0, LSE = -inf. window = None: no window (full causal attention with
    sinks). sinks of -inf give the bits of fa2_prefill_paged_varlen_window_bf16. C entry cln_fa2_prefill_paged_varlen_window_sink_bf16
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_window_sink_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, out, lse)


def fa2_decode_paged_multi_window_sink_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, out, lse=None, workspace=None):
    """fa2_decode_paged_multi_window_bf16 with attention sinks (sinks fp32 [Hq], the semantics of fa2_prefill_paged_varlen_window_sink_bf16), T in
    1 … 8; the sink enters once per row whatever the number of splits. window = None: no window. The plan and the workspace are those of
    fa2_decode_paged_multi_window_bf16. C entry cln_fa2_decode_paged_multi_window_sink_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, out, lse, workspace)


def fa2_decode_paged_multi_window_sink_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_bf16: what fa2_decode_paged_multi_window_bf16_plan returns;
    window = None: no window. C entry cln_fa2_decode_paged_multi_window_sink_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window)


def kv_append_paged_varlen_bf16_fp8(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, q=None, q_out=None,
                                    rope_table=None, rope="none"):
    """kv_append_paged_varlen_bf16 into a paged KV cache held in FP8: bf16 rows, torch.float8_e4m3fn pools [P,Hkv,page,D], k_scale / v_scale fp32
    [Hkv] (a stored byte c of KV head h means e4m3(c) * scale[h]); every element is e4m3(clamp(y / scale, +-448)) of the bf16 input or the fp32
    rotation result; q is rotated and written as bf16. C entry cln_kv_append_paged_varlen_bf16_fp8 (include/cln_amd_ext.h). Not a reference
    name."""
    from . import host
    return host.kv_append_paged_varlen_bf16_fp8(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, q, q_out, rope_table,
                                                rope)


def fa2_prefill_paged_varlen_window_sink_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window, sinks, out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_bf16 over a paged KV cache held in FP8 (torch.float8_e4m3fn pools, k_scale / v_scale fp32 [Hkv]): the
    bf16 entry's function on the dequantised pools. window = None: no window; sinks = None: no sink. C entry
    cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_window_sink_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window, sinks, out,
                                                              lse)


def fa2_decode_paged_multi_window_sink_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks, out, lse=None,
                                                workspace=None):
    """fa2_decode_paged_multi_window_sink_bf16 over a paged KV cache held in FP8 (torch.float8_e4m3fn pools, k_scale / v_scale fp32 [Hkv]), T in
    1 … 8. window = None: no window; sinks = None: no sink. The plan and the workspace are those of fa2_decode_paged_multi_window_bf16. C entry
    cln_fa2_decode_paged_multi_window_sink_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks, out, lse,
                                                            workspace)


def fa2_decode_paged_multi_window_sink_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_bf16_fp8: what fa2_decode_paged_multi_window_bf16_plan returns;
    window = None: no window. C entry cln_fa2_decode_paged_multi_window_sink_bf16_fp8_plan."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window)


def fa2_prefill_paged_varlen_window_sink_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_bf16 for any group size Hq / Hkv in 1 … 16 (Qwen2.5's 7, 5 and 6, Llama-3.2-3B's 3, 12, 16), not a
    power of two only; window = None: no window, sinks = None: no sink. For Hq / Hkv in {1, 2, 4, 8} the sibling's bits. C entry
    cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_window_sink_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, out, lse)


def fa2_decode_paged_multi_window_sink_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, out, lse=None, workspace=None):
    """fa2_decode_paged_multi_window_sink_bf16 for any group size Hq / Hkv in 1 … 16, T in 1 … 8 with T * Hq / Hkv <= 64; window = None: no
    window, sinks = None: no sink. C entry cln_fa2_decode_paged_multi_window_sink_anyg_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, out, lse, workspace)


def fa2_decode_paged_multi_window_sink_anyg_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_anyg_bf16: for Hq / Hkv in {1, 2, 4, 8} what
    fa2_decode_paged_multi_window_sink_bf16_plan returns; window = None: no window. C entry cln_fa2_decode_paged_multi_window_sink_anyg_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_anyg_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window)


def fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window, sinks, out,
                                                       lse=None):
    """fa2_prefill_paged_varlen_window_sink_bf16_fp8 for any group size Hq / Hkv in 1 … 16; window = None: no window, sinks = None: no sink. C
    entry cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window, sinks,
                                                                   out, lse)


def fa2_decode_paged_multi_window_sink_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks, out, lse=None,
                                                     workspace=None):
    """fa2_decode_paged_multi_window_sink_bf16_fp8 for any group size Hq / Hkv in 1 … 16, T in 1 … 8 with T * Hq / Hkv <= 64; window = None: no
    window, sinks = None: no sink. C entry cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks, out,
                                                                 lse, workspace)


def fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_anyg_bf16_fp8: what
    fa2_decode_paged_multi_window_sink_anyg_bf16_plan returns; window = None: no window. C entry
    cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window)


def fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, softmax_scale, softcap,
                                                           out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_anyg_bf16 with a softmax scale (None: 1 / sqrt(D); Gemma-2-27B 144 ** -0.5, Gemma-3-27B 168 ** -0.5,
    Granite's attention_multiplier) and logit soft-capping cap * tanh(score / cap) (None: no cap; Gemma-2 50, Grok-1 30), capped before the
    mask, the sink neither scaled nor capped. Both None: the any-G entry's bits. C entry cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks,
                                                                       softmax_scale, softcap, out, lse)


def fa2_decode_paged_multi_window_sink_softcap_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, softmax_scale, softcap, out,
                                                         lse=None, workspace=None):
    """fa2_decode_paged_multi_window_sink_anyg_bf16 with a softmax scale and logit soft-capping (as for
    fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16). C entry cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, softmax_scale,
                                                                     softcap, out, lse, workspace)


def fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_softcap_anyg_bf16: what
    fa2_decode_paged_multi_window_sink_anyg_bf16_plan returns; window = None: no window. C entry
    cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window)


def fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window, sinks,
                                                               softmax_scale, softcap, out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8 with a softmax scale and logit soft-capping (as for
    fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16; k_scale inside the tanh). C entry
    cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window,
                                                                           sinks, softmax_scale, softcap, out, lse)


def fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks,
                                                             softmax_scale, softcap, out, lse=None, workspace=None):
    """fa2_decode_paged_multi_window_sink_anyg_bf16_fp8 with a softmax scale and logit soft-capping (as for
    fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16; k_scale inside the tanh). C entry
    cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks,
                                                                         softmax_scale, softcap, out, lse, workspace)


def fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8: what
    fa2_decode_paged_multi_window_sink_anyg_bf16_plan returns; window = None: no window. C entry
    cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window)


def kv_append_paged_varlen_d256_bf16(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged_varlen_bf16 at head dim 256 (Gemma-2, Gemma-3): bf16 rows and pools [P,Hkv,page,256], all three rope modes, the half-split
    pairs (i, i + 128); any other head dim is refused. C entry cln_kv_append_paged_varlen_d256_bf16 (include/cln_amd_ext.h). Not a reference
    name."""
    from . import host
    return host.kv_append_paged_varlen_d256_bf16(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q, q_out, rope_table, rope)


def fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, softmax_scale,
                                                                softcap, out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16 at head dim 256 (Gemma-2-2B / 9B: cap 50, window 4096; Gemma-3-1B / 4B / 12B): the
    same arguments and semantics, D = 256 only. C entry cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16 (include/cln_amd_ext.h).
    Not a reference name."""
    from . import host
    return host.fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks,
                                                                            softmax_scale, softcap, out, lse)


def fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, softmax_scale, softcap,
                                                              out, lse=None, workspace=None):
    """fa2_decode_paged_multi_window_sink_softcap_anyg_bf16 at head dim 256: the same arguments and semantics, D = 256 only, T in 1 … 8 with
    T * Hq / Hkv <= 32; the workspace is sized by fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan. C entry
    cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, softmax_scale,
                                                                          softcap, out, lse, workspace)


def fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16: the entry's own plan (key step 64, D = 256);
    window = None: no window. C entry cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window)


def fa2_decode_paged_mla_bf16(q, pool, block_table, seqlens, softmax_scale, out, lse=None, workspace=None):
    """Multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2) decode over a paged latent cache: q bf16 [B,T,Hq,576], already absorbed
    (q_nope W_UK | q_pe); pool bf16 [P,page,576] of rows [c 512 | k_pe 64], each the key (576 dims) and the value (dims 0 … 511) of every head;
    out bf16 [B,T,Hq,512] in latent space; lse fp32 [B,T,Hq] or None. softmax_scale is required (finite, > 0). T in 1 … 8, Hq in 1 … 128; the
    workspace is sized by fa2_decode_paged_mla_bf16_plan. C entry cln_fa2_decode_paged_mla_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_mla_bf16(q, pool, block_table, seqlens, softmax_scale, out, lse, workspace)


def fa2_decode_paged_mla_bf16_plan(B, T, Hq, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_bf16: a function of these five numbers only (row groups of 64 query rows, key
    step 64, D = 512). C entry cln_fa2_decode_paged_mla_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_mla_bf16_plan(B, T, Hq, max_pages, page)


def kv_append_paged_mla_bf16(c_new, k_pe_new, pool, block_table, seqlens, cu_q, q=None, q_out=None, rope_table=None, rope="none"):
    """Append a packed batch of latent rows to the paged latent cache of fa2_decode_paged_mla_bf16: c_new bf16 [total_q,512] copied bit for bit,
    k_pe_new bf16 [total_q,64] rotated at the token's position; q / q_out bf16 [total_q,Hq,576] alike (dims 0 … 511 copied, 512 … 575 rotated);
    rope_table fp32 [max_pos,64] (kv_append_rope_table(max_pos, 64)); rope "none", "half" (pairs (i, i + 32)) or "interleaved". C entry
    cln_kv_append_paged_mla_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.kv_append_paged_mla_bf16(c_new, k_pe_new, pool, block_table, seqlens, cu_q, q, q_out, rope_table, rope)


def fa2_prefill_varlen_mla_bf16(q, kv, k_pe, cu_q, cu_k, softmax_scale, out, lse=None, causal=True):
    """Multi-head latent attention prefill (un-absorbed: key 192 = 128 nope + 64 rotary dims, value 128, Hkv = Hq) of a packed batch: q bf16
    [total_q,Hq,192], kv bf16 [total_k,Hq,256] = [k_nope | v] as kv_b_proj writes it, k_pe bf16 [total_k,64] shared by every head, cu_q / cu_k
    int32 [B+1] on the GPU, out bf16 [total_q,Hq,128], lse fp32 [total_q,Hq] or None. causal=True: query t sees the keys j < L_b - (T_b - 1 - t);
    False: all L_b (a context chunk). softmax_scale is required (finite, > 0). Hq in 1 … 128. C entry cln_fa2_prefill_varlen_mla_bf16
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_prefill_varlen_mla_bf16(q, kv, k_pe, cu_q, cu_k, softmax_scale, out, lse, causal)


def attn_merge_states_bf16(o_a, lse_a, o_b, lse_b, out, lse=None):
    """Merge two attention states over disjoint key sets (chunked prefill): o_a, o_b bf16 [..., D], lse_a, lse_b fp32 [...], out bf16 (may be
    o_a), lse fp32 or None (may be lse_a); D % 8 == 0, 8 <= D <= 512. A side whose LSE is -inf is selected out; both -inf give O = 0, LSE =
    -inf. C entry cln_attn_merge_states_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.attn_merge_states_bf16(o_a, lse_a, o_b, lse_b, out, lse)


def kv_gather_paged_mla_bf16(pool, block_table, cu_k, out, starts=None):
    """Gather latent rows out of the paged latent cache into a packed batch, the mirror of kv_append_paged_mla_bf16: pool bf16 [P,page,576],
    block_table int32 [B,max_pages], cu_k int32 [B+1], starts int32 [B] or None (0), out bf16 [total_k,576]; packed row cu_k[b] + i = cache row
    starts[b] + i, bit for bit; rows at or past max_pages * page are zeros. C entry cln_kv_gather_paged_mla_bf16 (include/cln_amd_ext.h). Not a
    reference name."""
    from . import host
    return host.kv_gather_paged_mla_bf16(pool, block_table, cu_k, out, starts)


def fa2_decode_paged_mla_bf16_fp8(q, pool, block_table, seqlens, kv_scale, softmax_scale, out, lse=None, workspace=None):
    """fa2_decode_paged_mla_bf16 over a latent cache held in FP8: pool torch.float8_e4m3fn [P,page,576] of rows [c 512 | k_pe 64] in codes,
    kv_scale fp32 [1] on the GPU (one scale for the whole pool: value = e4m3(code) * kv_scale); q bf16 [B,T,Hq,576], out bf16 [B,T,Hq,512], lse
    fp32 [B,T,Hq] or None, softmax_scale required. The workspace is sized by fa2_decode_paged_mla_bf16_fp8_plan. C entry
    cln_fa2_decode_paged_mla_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_mla_bf16_fp8(q, pool, block_table, seqlens, kv_scale, softmax_scale, out, lse, workspace)


def fa2_decode_paged_mla_bf16_fp8_plan(B, T, Hq, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_bf16_fp8: exactly fa2_decode_paged_mla_bf16_plan's. C entry
    cln_fa2_decode_paged_mla_bf16_fp8_plan."""
    from . import host
    return host.fa2_decode_paged_mla_bf16_fp8_plan(B, T, Hq, max_pages, page)


def kv_append_paged_mla_bf16_fp8(c_new, k_pe_new, pool, block_table, seqlens, cu_q, kv_scale, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged_mla_bf16 into a latent cache held in FP8: pool torch.float8_e4m3fn [P,page,576], kv_scale fp32 [1] on the GPU; the byte of
    an element is e4m3(clamp(y * (1 / kv_scale), ±448)) in fp32, round to nearest even, y the bf16 input or the fp32 rotation result; q / q_out
    stay bf16. C entry cln_kv_append_paged_mla_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.kv_append_paged_mla_bf16_fp8(c_new, k_pe_new, pool, block_table, seqlens, cu_q, kv_scale, q, q_out, rope_table, rope)


def kv_gather_paged_mla_bf16_fp8(pool, block_table, cu_k, kv_scale, out, starts=None):
    """kv_gather_paged_mla_bf16 out of a latent cache held in FP8: pool torch.float8_e4m3fn [P,page,576], kv_scale fp32 [1] on the GPU, out bf16
    [total_k,576], each element bf16(fp32(code) * kv_scale) with one rounding. C entry cln_kv_gather_paged_mla_bf16_fp8
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.kv_gather_paged_mla_bf16_fp8(pool, block_table, cu_k, kv_scale, out, starts)


def fa2_decode_paged_mla_sparse_bf16(q, pool, block_table, seqlens, indices, softmax_scale, out, lse=None, workspace=None):
    """Sparse MLA decode (DeepSeek-V3.2) over the paged latent cache of fa2_decode_paged_mla_bf16: q bf16 [B,T,Hq,576] absorbed, pool bf16
    [P,page,576], out bf16 [B,T,Hq,512], lse fp32 [B,T,Hq] or None, softmax_scale required, any T >= 1. indices int32 [B,T,topk] on the GPU: per
    query token the logical token positions it attends to, shared by its heads; a slot is valid iff 0 <= idx < seqlens[b] - (T - 1 - t) (the
    length clamped to the cache), every other value (-1 …) is an empty slot that may stand anywhere. Pass distinct positions: one listed twice is
    two keys. No valid slot: O = 0, LSE = -inf. The workspace is sized by fa2_decode_paged_mla_sparse_bf16_plan. C entry
    cln_fa2_decode_paged_mla_sparse_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.fa2_decode_paged_mla_sparse_bf16(q, pool, block_table, seqlens, indices, softmax_scale, out, lse, workspace)


def fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, topk, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_sparse_bf16: the splits divide the topk index slots of a query token. C entry
    cln_fa2_decode_paged_mla_sparse_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, topk, max_pages, page)


def kv_append_paged_index_bf16(k_idx_new, idx_pool, block_table, seqlens, cu_q):
    """Append the index keys of DeepSeek-V3.2's indexer to their paged cache: k_idx_new bf16 [total_q,128], idx_pool bf16 [P,page,128] behind the
    block table of the latent cache, the packed convention, seqlens after the append and liveness as in kv_append_paged_mla_bf16; rows copied
    bit for bit. No rope argument: the model rotates the key, then applies a Hadamard transform, before it caches it. C entry
    cln_kv_append_paged_index_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.kv_append_paged_index_bf16(k_idx_new, idx_pool, block_table, seqlens, cu_q)


def mla_index_logits_paged_bf16(q_idx, weights, idx_pool, block_table, seqlens, logits):
    """The indexer's logits over the paged index-key cache: q_idx bf16 [B,T,Hi,128], weights fp32 [B,T,Hi], idx_pool bf16 [P,page,128], logits
    fp32 [B,T,ld]; logits[b,t,j] = sum_h weights[b,t,h] * max(0, q_idx[b,t,h] . k_idx[j]) for 0 <= j < vis(b,t) =
    clamp(seqlens[b], 0, min(max_pages * page, ld)) - (T - 1 - t), nothing else written or read. Any T >= 1, Hi in 1 … 64. C entry
    cln_mla_index_logits_paged_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.mla_index_logits_paged_bf16(q_idx, weights, idx_pool, block_table, seqlens, logits)


def mla_index_topk(logits, seqlens, topk, indices):
    """The indexer's exact top-k: logits fp32 [B,T,ld], indices int32 [B,T,topk]; per (b,t) the topk visible positions first under (logit
    descending, position ascending), written in ascending position order, or the dense list [0 … n-1, -1 …] when n <= topk: the list
    fa2_decode_paged_mla_sparse_bf16 takes. C entry cln_mla_index_topk (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.mla_index_topk(logits, seqlens, topk, indices)


def index_pool_fp8_views(idx_pool):
    """(codes, scales) of an FP8 index pool torch.uint8 [P,page,132]: codes float8_e4m3fn [P,page,128] (slot r at byte 128 * r of its page) and
    scales float32 [P,page] (at byte 128 * page + 4 * r), views of the same storage, no copy; value = e4m3(code) * scale. Not a reference
    name."""
    from . import host
    return host.index_pool_fp8_views(idx_pool)


def kv_append_paged_index_bf16_fp8(k_idx_new, idx_pool, block_table, seqlens, cu_q, scale_pow2=False):
    """kv_append_paged_index_bf16 into an index-key cache held in FP8 with one fp32 scale per token (DeepSeek-V3.2's own format, 132 bytes a
    token): idx_pool uint8 [P,page,132] in the layout of index_pool_fp8_views; per live token scale = max(amax, 1e-4) / 448 in fp32, rounded up
    to a power of two with scale_pow2 (ue8m0), code = e4m3fn(clamp(k / scale, ±448)); every other byte keeps its value. C entry
    cln_kv_append_paged_index_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.kv_append_paged_index_bf16_fp8(k_idx_new, idx_pool, block_table, seqlens, cu_q, scale_pow2)


def mla_index_logits_paged_bf16_fp8(q_idx, weights, idx_pool, block_table, seqlens, logits):
    """mla_index_logits_paged_bf16 over the FP8 index pool uint8 [P,page,132]: logits[b,t,j] = s_j * sum_h weights[b,t,h] *
    max(0, q_idx[b,t,h] . c_j) for 0 <= j < vis(b,t), c_j the codes read as numbers and s_j the token's scale (finite and >= 0), nothing else
    written or read; q_idx bf16, weights and logits fp32, any T >= 1, Hi in 1 … 64. C entry cln_mla_index_logits_paged_bf16_fp8
    (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.mla_index_logits_paged_bf16_fp8(q_idx, weights, idx_pool, block_table, seqlens, logits)


def fa2_decode_paged_mla_sparse_bf16_fp8(q, pool, block_table, seqlens, kv_scale, indices, softmax_scale, out, lse=None, workspace=None):
    """fa2_decode_paged_mla_sparse_bf16 over a latent cache held in FP8 (a DeepSeek-V3.2 step on the pool kv_append_paged_mla_bf16_fp8 writes):
    pool torch.float8_e4m3fn [P,page,576] of rows [c 512 | k_pe 64] in codes, kv_scale fp32 [1] on the GPU (one scale for the whole pool: value
    = e4m3(code) * kv_scale); q bf16 [B,T,Hq,576] absorbed, indices int32 [B,T,topk] on the GPU with the validity rule, the empty slots and the
    duplicates of the bf16 entry, out bf16 [B,T,Hq,512], lse fp32 [B,T,Hq] or None, softmax_scale required, any T >= 1. The workspace is sized
    by fa2_decode_paged_mla_sparse_bf16_fp8_plan. C entry cln_fa2_decode_paged_mla_sparse_bf16_fp8 (include/cln_amd_ext.h). Not a reference
    name."""
    from . import host
    return host.fa2_decode_paged_mla_sparse_bf16_fp8(q, pool, block_table, seqlens, kv_scale, indices, softmax_scale, out, lse, workspace)


def fa2_decode_paged_mla_sparse_bf16_fp8_plan(B, T, Hq, topk, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_sparse_bf16_fp8: exactly fa2_decode_paged_mla_sparse_bf16_plan's. C entry
    cln_fa2_decode_paged_mla_sparse_bf16_fp8_plan."""
    from . import host
    return host.fa2_decode_paged_mla_sparse_bf16_fp8_plan(B, T, Hq, topk, max_pages, page)


def mla_index_logits_paged_varlen_bf16(q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits):
    """mla_index_logits_paged_bf16 for a packed batch: q_idx bf16 [total_q,Hi,128], weights fp32 [total_q,Hi], logits fp32
    [total_q,ld], cu_q int32 [B+1] on the GPU; packed row r = cu_q[b] + t has vis(r) = clamp(seqlens[b], 0, cap) - (T_b - 1 - t),
    T_b = cu_q[b+1] - cu_q[b]; a row of no sequence writes nothing. With cu_q = [0, T, 2T, …] the fixed-T entry's bits. C entry
    cln_mla_index_logits_paged_varlen_bf16 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.mla_index_logits_paged_varlen_bf16(q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits)


def mla_index_logits_paged_varlen_bf16_fp8(q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits):
    """mla_index_logits_paged_bf16_fp8 for a packed batch: the FP8 index pool uint8 [P,page,132], everything else as in
    mla_index_logits_paged_varlen_bf16. C entry cln_mla_index_logits_paged_varlen_bf16_fp8 (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.mla_index_logits_paged_varlen_bf16_fp8(q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits)


def mla_index_topk_varlen(logits, seqlens, cu_q, topk, indices):
    """mla_index_topk for a packed batch: logits fp32 [total_q,ld], cu_q int32 [B+1] on the GPU, indices int32 [total_q,topk], every slot of
    every row written; n = max(clamp(seqlens[b], 0, ld) - (T_b - 1 - t), 0) for packed row r = cu_q[b] + t, a row of no sequence all -1. C
    entry cln_mla_index_topk_varlen (include/cln_amd_ext.h). Not a reference name."""
    from . import host
    return host.mla_index_topk_varlen(logits, seqlens, cu_q, topk, indices)


def fa2_decode_paged_mla_sparse_varlen_bf16(q, pool, block_table, seqlens, cu_q, indices, softmax_scale, out, lse=None, workspace=None):
    """fa2_decode_paged_mla_sparse_bf16 for a packed batch: q bf16 [total_q,Hq,576], indices int32 [total_q,topk], out bf16 [total_q,Hq,512],
    lse fp32 [total_q,Hq] or None, cu_q int32 [B+1] on the GPU; a slot of packed row r = cu_q[b] + t is valid iff 0 <= idx < vis(r) =
    clamp(seqlens[b], 0, max_pages * page) - (T_b - 1 - t); a row of no sequence gets O = 0, LSE = -inf. The workspace is sized by
    fa2_decode_paged_mla_sparse_varlen_bf16_plan. C entry cln_fa2_decode_paged_mla_sparse_varlen_bf16 (include/cln_amd_ext.h). Not a
    reference name."""
    from . import host
    return host.fa2_decode_paged_mla_sparse_varlen_bf16(q, pool, block_table, seqlens, cu_q, indices, softmax_scale, out, lse, workspace)


def fa2_decode_paged_mla_sparse_varlen_bf16_plan(total_q, Hq, topk, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_sparse_varlen_bf16: fa2_decode_paged_mla_sparse_bf16_plan with total_q in the
    place of B * T. C entry cln_fa2_decode_paged_mla_sparse_varlen_bf16_plan."""
    from . import host
    return host.fa2_decode_paged_mla_sparse_varlen_bf16_plan(total_q, Hq, topk, max_pages, page)


def fa2_decode_paged_mla_sparse_varlen_bf16_fp8(q, pool, block_table, seqlens, cu_q, kv_scale, indices, softmax_scale, out, lse=None,
                                                workspace=None):
    """fa2_decode_paged_mla_sparse_bf16_fp8 for a packed batch: pool torch.float8_e4m3fn [P,page,576], kv_scale fp32 [1] on the GPU, everything
    else as in fa2_decode_paged_mla_sparse_varlen_bf16. C entry cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8 (include/cln_amd_ext.h). Not a
    reference name."""
    from . import host
    return host.fa2_decode_paged_mla_sparse_varlen_bf16_fp8(q, pool, block_table, seqlens, cu_q, kv_scale, indices, softmax_scale, out, lse,
                                                            workspace)


def fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan(total_q, Hq, topk, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_sparse_varlen_bf16_fp8: exactly
    fa2_decode_paged_mla_sparse_varlen_bf16_plan's. C entry cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan."""
    from . import host
    return host.fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan(total_q, Hq, topk, max_pages, page)


def fa2_attention(q, k, v, causal=False):
    """Differentiable FlashAttention-2 (scale 1/sqrt(D)), layout [B,H,N,D] as torch.nn.functional.scaled_dot_product_attention:
    fp16, D in {64, 128}, N % 256 == 0. Forward fa2_fwd_lse, backward fa2_bwd."""
    return _attention_fn().apply(q, k, v, bool(causal))


_ATTN_FN = None


def _attention_fn():
    global _ATTN_FN
    if _ATTN_FN is None:
        import torch

        class FA2Attention(torch.autograd.Function):
            @staticmethod
            def forward(ctx, q, k, v, causal):
                q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
                o = torch.empty_like(q)
                lse = torch.empty(q.shape[:3], dtype=torch.float32, device=q.device)
                fa2_fwd_lse(q, k, v, o, lse, causal)
                ctx.save_for_backward(q, k, v, o, lse)
                ctx.causal = causal
                return o

            @staticmethod
            def backward(ctx, grad_out):
                q, k, v, o, lse = ctx.saved_tensors
                dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
                fa2_bwd(q, k, v, o, grad_out.contiguous(), lse, dq, dk, dv, causal=ctx.causal)
                return dq, dk, dv, None

        _ATTN_FN = FA2Attention
    return _ATTN_FN
