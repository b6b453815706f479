/* cln_amd_ext.h -- C ABI entry points beyond the reference surface of cln_amd.h (hand-written; cln_amd.h is generated
 * from manifest.py and carries the reference names only). Same conventions and status codes as cln_amd.h.
 */
#ifndef CLN_AMD_EXT_H
#define CLN_AMD_EXT_H
#include "cln_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Causal FlashAttention-2 forward: O[b,h,i,:] = sum_{j <= i} softmax_j(Q_i . K_j / sqrt(D)) V_j.
 * q, k, v, o: fp16 [B,H,N,D], contiguous, 16-byte aligned; one sequence length, so the mask is key <= query (top-left).
 * Supported: D in {64, 128}, N a multiple of 256. stages = 1: every tile fetch waited for where it is issued; any other
 * value: the pipelined form. Both forms give bit-identical results.
 * Returns 0, -1 (null / misaligned pointer, non-positive B, H, N or D), -2 (other D, N % 256 != 0) -- both checked before
 * any device access -- or -3 (launch error). cln_describe("cln_fa2_fwd_causal", B, H, N, D, stages, ...) names the kernel.
 */
int cln_fa2_fwd_causal(const void* q, const void* k, const void* v, void* o, int B, int H, int N, int D, int stages, void* stream);

/* ---- Forwards that also write the row log-sum-exp, the input of the backward below (non-causal / causal).
 * lse: fp32 [B,H,N], 16-byte aligned; lse[b,h,i] = ln sum_{j allowed} exp(Q_i . K_j / sqrt(D)) (natural log). O is bit-identical to
 * cln_fa2_fwd_causal (causal) and to the plain 32-rows-per-wave kernel (non-causal). Same support, stages and statuses as
 * cln_fa2_fwd_causal; -1 also when o or lse equals an input pointer or each other. cln_describe names the kernel.
 */
int cln_fa2_fwd_lse(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int D, int stages, void* stream);
int cln_fa2_fwd_causal_lse(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int D, int stages, void* stream);

/* ---- FlashAttention-2 backward (non-causal / causal; the mask as in the forward): dq, dk, dv (fp16 [B,H,N,D]) from q, k, v, o, dout
 * (fp16 [B,H,N,D]) and lse (fp32 [B,H,N], from cln_fa2_fwd_lse / cln_fa2_fwd_causal_lse). delta: caller-provided fp32 [B,H,N]
 * scratch, written with rowsum(dout o o) and read back by the second kernel. Two kernels on `stream`; every output element is summed
 * by one workgroup in a fixed order, so results are bit-repeatable.
 * Supported: D in {64, 128}, N a multiple of 256. Returns 0, -1 (null / misaligned pointer, non-positive B, H, N or D, an output
 * pointer equal to an input pointer or to another output), -2 (other D, N % 256 != 0, grid too large) -- both checked before any
 * device access -- or -3 (launch error). cln_describe names both kernels; the stages argument is ignored.
 */
int cln_fa2_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta,
                void* dq, void* dk, void* dv, int B, int H, int N, int D, void* stream);
int cln_fa2_bwd_causal(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta,
                       void* dq, void* dk, void* dv, int B, int H, int N, int D, void* stream);

/* ---- Single-query ("decode") attention over a KV cache: O[b,h,:] = sum_{j < len_b} softmax_j(q . K_j / sqrt(D)) V_j.
 * q, o: fp16 [B,H,D]; k_cache, v_cache: fp16 [B,H,Nmax,D] contiguous; seqlens: int32 [B] ON THE DEVICE (the host never reads it: no sync, the call can
 * be captured in a graph); lse: fp32 [B,H] (natural log) or NULL. The kernels clamp each length to [0, Nmax]; a clamped length of 0 gives O = 0 and
 * LSE = -inf. No cache row at index >= min(len_b, Nmax) is read. Supported: D in {64, 128}; Nmax is any positive number.
 * cln_fa2_decode_plan: the split of the keys this (B, H, Nmax, D) runs with -- *splits chunks of *chunk keys per head -- and the bytes of workspace
 * the call needs: B H splits (D + 2) 4 when splits > 1, else 0 (a NULL workspace is then accepted). The plan depends on nothing else, so the bits of
 * a sequence do not depend on the lengths of its neighbours. The library allocates nothing; results are bit-repeatable (no atomics).
 * Returns 0, -1 (null q / k_cache / v_cache / seqlens / o; a q, k_cache, v_cache, o, lse or workspace pointer that is not 16-byte aligned or a seqlens
 * pointer that is not 4-byte aligned; non-positive B, H, Nmax or D; o, lse or workspace equal to an input or to each other; splits > 1 with a NULL
 * workspace or workspace_bytes below the plan's), -2 (other D, grid too large) -- all checked before any device access -- or -3 (launch error).
 * cln_describe("cln_fa2_decode", B, H, Nmax, D, stages, ...) names the kernels and the plan; the stages argument is ignored.
 */
int cln_fa2_decode_plan(int B, int H, int Nmax, int D, int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode(const void* q, const void* k_cache, const void* v_cache, const int* seqlens, void* o, float* lse,
                   void* workspace, long long workspace_bytes, int B, int H, int Nmax, int D, void* stream);

/* ---- Decode attention over a PAGED KV cache with grouped query heads (GQA / MQA):
 *   O[b,h,:] = sum_{j < len_b} softmax_j(q[b,h] . K_j / sqrt(D)) V_j, where key j of sequence b and query head h is row j % page of KV head h / G in
 *   the physical page block_table[b, j / page], G = Hq / Hkv.
 * q, o: fp16 [B,Hq,D]; k_pages, v_pages: fp16 [P,Hkv,page,D] contiguous (one pool of P pages, the rows of one head in one page consecutive);
 * block_table: int32 [B,max_pages] and seqlens: int32 [B], both ON THE DEVICE (the host reads neither: no sync, the call can be captured in a graph
 * and replayed after the table, the lengths and the cache have changed); lse: fp32 [B,Hq] (natural log) or NULL.
 * Supported: D in {64, 128}; Hq = G Hkv with G in {1, 2, 4, 8}; page in {16, 32, 64, 128, 256}; any P >= 1 and max_pages >= 1 with
 * max_pages page < 2^31. The kernels clamp each length to [0, max_pages page]; a clamped length of 0 gives O = 0 and LSE = -inf.
 * Of a sequence only the table entries 0 .. ceil(len_b / page) - 1 are read, and only the rows < len_b of the pages they name: entries past that and
 * pool pages that no live entry names may hold anything. THE LIVE ENTRIES MUST LIE IN [0, P): the kernels do not check them -- that is the caller's
 * contract, like the pointers (P itself is only checked to be positive). One workgroup serves all G query heads of a KV head, so every K and V row is
 * read once per KV head.
 * cln_fa2_decode_paged_plan: the split this (B, Hq, Hkv, max_pages, page, D) runs with -- *splits chunks of *chunk keys (a multiple of the page) --
 * and the bytes of workspace the call needs: B Hq splits (D + 2) 4 when splits > 1, else 0 (a NULL workspace is then accepted). The plan depends on
 * nothing else, so the bits of a sequence depend neither on its neighbours nor on where its pages lie. The library allocates nothing; results are
 * bit-repeatable (no atomics).
 * Returns 0, -1 (null q / k_pages / v_pages / block_table / seqlens / o; a q, k_pages, v_pages, o, lse or workspace pointer that is not 16-byte
 * aligned or a block_table / seqlens pointer that is not 4-byte aligned; non-positive B, Hq, Hkv, P, max_pages, page or D; Hq % Hkv != 0; o, lse or
 * workspace equal to an input or to each other; splits > 1 with a NULL workspace or workspace_bytes below the plan's), -2 (other D, G or page,
 * max_pages page >= 2^31, grid too large) -- all checked before any device access -- or -3 (launch error).
 * cln_fa2_decode_paged_describe writes the kernel instantiations and the plan as text into buf (at most len bytes, NUL-terminated) and returns the
 * text's length, or the same -1 / -2 (cln_describe carries four dims only, so this entry has its own).
 */
int cln_fa2_decode_paged_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens, void* o, float* lse,
                         void* workspace, long long workspace_bytes, int B, int Hq, int Hkv, int P, int max_pages, int page, int D, void* stream);
int cln_fa2_decode_paged_describe(int B, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);

/* ---- Multi-token decode attention (speculative verify, short chunked appends) over the same PAGED KV cache, on the matrix cores:
 *   O[b,t,h,:] = sum_{j < n(b,t)} softmax_j(q[b,t,h] . K_j / sqrt(D)) V_j,  n(b,t) = len_b - (T - 1 - t),
 *   keys through the block table exactly as for cln_fa2_decode_paged. len_b = clamp(seqlens[b], 0, max_pages page) counts the keys of sequence b
 *   INCLUDING its T newest tokens, whose K / V rows the caller has already written: query t is the token at position len_b - T + t and sees itself
 *   and everything before it. n(b,t) <= 0 (possible when len_b < T) gives O = 0 and LSE = -inf for that query.
 * q, o: fp16 [B,T,Hq,D]; k_pages, v_pages: fp16 [P,Hkv,page,D]; block_table: int32 [B,max_pages] and seqlens: int32 [B], both ON THE DEVICE and never
 * read by the host; lse: fp32 [B,T,Hq] (natural log) or NULL.
 * Supported: T in 1 .. 8; D, G = Hq / Hkv, page, P and max_pages as for cln_fa2_decode_paged. Of a sequence only the table entries
 * 0 .. ceil(len_b / page) - 1 are read, and only the rows < len_b of the pages they name; THE LIVE ENTRIES MUST LIE IN [0, P). One workgroup serves
 * all T G query rows of a KV head, so every K and V row is read once per KV head and call, whatever T is.
 * cln_fa2_decode_paged_multi_plan: the split this (B, T, Hq, Hkv, max_pages, page, D) runs with -- *splits chunks of *chunk keys (a multiple of
 * max(page, 128)) -- and the bytes of workspace the call needs: B T Hq splits (D + 2) 4 when splits > 1, else 0 (a NULL workspace is then
 * accepted). The plan depends on nothing else, so the bits of a sequence depend neither on its neighbours nor on where its pages lie. The library
 * allocates nothing; results are bit-repeatable (no atomics).
 * Returns 0, -1 (as cln_fa2_decode_paged, with T among the dimensions that must be positive), -2 (T > 8; other D, G or page; max_pages page >= 2^31;
 * grid too large) -- all checked before any device access -- or -3 (launch error).
 * cln_fa2_decode_paged_multi_describe writes the kernel instantiations and the plan as text into buf (at most len bytes, NUL-terminated) and returns
 * the text's length, or the same -1 / -2.
 */
int cln_fa2_decode_paged_multi_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk,
                                    long long* workspace_bytes);
int cln_fa2_decode_paged_multi(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens, void* o,
                               float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages, int page,
                               int D, void* stream);
int cln_fa2_decode_paged_multi_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);

/* ---- Append to the same PAGED KV cache, with the rotary embedding fused in: the part of a decode step in front of the attention call, as one
 * launch with no workspace. seqlens[b] counts the T new tokens, exactly as for cln_fa2_decode_paged_multi, so the same tensor feeds the attention
 * call that follows on the same stream. Token t of sequence b stands at pos = seqlens[b] - T + t (formed in 64 bits: any int32 value is safe) and is
 * LIVE iff 0 <= pos < max_pages page and, with a rotation, pos < max_pos. For every KV head h a live token's rows go to
 *   k_pages[block_table[b, pos / page], h, pos % page, :] = rot(k_new[b,t,h,:]),   v_pages[same place] = v_new[b,t,h,:] (never rotated),
 * and q_out[b,t,h,:] = rot(q[b,t,h,:]). A token that is not live writes nothing to the pools, and its q_out rows are written as zeros.
 * k_new, v_new: fp16 [B,T,Hkv,D]; k_pages, v_pages: fp16 [P,Hkv,page,D], written in place; block_table: int32 [B,max_pages] and seqlens: int32 [B],
 * both ON THE DEVICE and never read by the host; q: fp16 [B,T,Hq,D] or NULL; q_out: fp16 [B,T,Hq,D] or NULL;
 * rope_table: fp32 [max_pos,D] or NULL, row p = cos(p f_0) .. cos(p f_{D/2-1}), then sin(p f_0) .. sin(p f_{D/2-1}).
 * rope_mode 0: none -- K and V are copied bit for bit; q, q_out and rope_table must all be NULL. 1: half-split pairs (i, i + D/2) (NeoX / Llama).
 * 2: interleaved pairs (2i, 2i + 1). For 1 and 2, pair i of a live token becomes (x1 c - x2 s, x1 s + x2 c) with c = rope_table[pos, i] and
 * s = rope_table[pos, D/2 + i]: products and sums in fp32, one rounding to fp16 at the store; full width only. It is applied to K and, when q and
 * q_out are given (together, or both NULL), to q. q_out == q is allowed; every other equality among k_pages, v_pages, q_out or between one of them
 * and an input is rejected.
 * Read: seqlens[b], the entry block_table[b, pos / page] and row pos of rope_table of live tokens, and the new rows. Written: the live rows only;
 * every other byte of both pools is untouched. THE CALLER'S CONTRACT, not checked: the live entries lie in [0, P), and no two live (sequence, page
 * index) pairs name the same physical page.
 * Supported: D in {64, 128}; page in {16, 32, 64, 128, 256}; any Hq that is a multiple of Hkv; any T >= 1 (a prompt chunk is appended with the same
 * call); any B, P, max_pages >= 1 with max_pages page < 2^31. Deterministic, no atomics, no library state.
 * Returns 0, -1 (null k_new / v_new / k_pages / v_pages / block_table / seqlens; the pointer rules of rope_mode; a tensor pointer that is not 16-byte
 * aligned or a block_table / seqlens / rope_table pointer that is not 4-byte aligned; a non-positive dimension, or max_pos <= 0 with a rotation;
 * Hq % Hkv != 0; forbidden aliasing), -2 (other D, page or rope_mode; max_pages page >= 2^31; a grid that does not fit) -- all checked before any
 * device access -- or -3 (launch error).
 * cln_kv_append_paged_describe writes the kernel instantiation and the launch as text into buf (at most len bytes, NUL-terminated; with a rotation
 * it counts the q rows) and returns the text's length, or the same -1 / -2.
 */
int cln_kv_append_paged(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table, const int* seqlens,
                        const void* q, void* q_out, const float* rope_table, int B, int T, int Hq, int Hkv, int P, int max_pages, int page, int D,
                        int max_pos, int rope_mode, void* stream);
int cln_kv_append_paged_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode, char* buf, int len);

/* ---- Prefill attention over the same PAGED KV cache: the semantics of cln_fa2_decode_paged_multi with T unbounded, for a prompt or a chunk of one
 * that cln_kv_append_paged has written. q, o: fp16 [B,T,Hq,D]; k_pages, v_pages, block_table, seqlens as for cln_fa2_decode_paged; lse: fp32
 * [B,T,Hq] or NULL. len_b = clamp(seqlens[b], 0, max_pages page) counts the T newest tokens, and
 *   o[b,t,h,:] = sum_{j < n(b,t)} softmax_j(q[b,t,h,:] . K_j / sqrt(D)) V_j,   n(b,t) = len_b - (T - 1 - t);
 * n(b,t) <= 0 gives o = 0 and lse = -inf. A sequence with len_b < T therefore has its live tokens right-aligned, exactly as cln_kv_append_paged
 * treats it: that is how a ragged prefill batch is expressed. Scores and softmax statistics in fp32, P rounded to fp16 for the second product.
 * Supported: any T >= 1; D in {64, 128}; G = Hq / Hkv in {1, 2, 4, 8}; page in {16, 32, 64, 128, 256}; max_pages page < 2^31. Of a sequence only
 * the table entries 0 .. ceil(len_b / page) - 1 are read, and only the rows < len_b of the pages they name; THE LIVE ENTRIES MUST LIE IN [0, P).
 * One launch, no workspace, no split over the keys, no atomics: a workgroup owns 128 consecutive query rows r = t G + g of a (sequence, KV head)
 * and walks the keys below the causal edge of its last token in steps of 64, so a sequence's bits depend neither on its neighbours nor on where
 * its pages lie. T <= 8 is also served by cln_fa2_decode_paged_multi, which splits the keys and is the entry for few rows over a long context;
 * the two agree within tolerance, not in bits.
 * Returns 0, -1 (a NULL q, k_pages, v_pages, block_table, seqlens or o; one of q, k_pages, v_pages, o not 16-byte aligned or block_table, seqlens,
 * lse not 4-byte aligned; a non-positive dimension; Hq % Hkv != 0; o or lse equal to an input or to each other), -2 (other D, G or page;
 * max_pages page >= 2^31; a grid that does not fit) -- all checked before any device access -- or -3 (launch error).
 * cln_fa2_prefill_paged_describe writes the kernel instantiation, its tile geometry (rows= and keys=) and the grid as text into buf (at most len
 * bytes, NUL-terminated) and returns the text's length, or the same -1 / -2.
 */
int cln_fa2_prefill_paged(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens, void* o, float* lse,
                          int B, int T, int Hq, int Hkv, int P, int max_pages, int page, int D, void* stream);
int cln_fa2_prefill_paged_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);

/* ---- The same PAGED KV cache held in FP8: a quantising append (the writer) and single-query decode attention (the reader).
 * k_pages, v_pages: one byte per element, [P,Hkv,page,D] contiguous, OCP e4m3fn (torch.float8_e4m3fn; max finite 448; NOT the fnuz encoding of
 * gfx942). k_scale, v_scale: fp32 [Hkv], one scale per KV head, ON THE DEVICE and never read by the host (a per-tensor scale is the same value
 * repeated). A stored byte c of KV head h means the real value e4m3(c) * scale[h]. block_table, seqlens, the page sizes, D, the liveness rules and
 * the caller's contracts are exactly those of cln_kv_append_paged and cln_fa2_decode_paged. THE CALLER'S CONTRACT, not checked on the device: every
 * scale is finite and > 0, the new rows are finite, and no live byte of the pools is a NaN code (0x7f, 0xff; the append never writes one).
 *
 * cln_kv_append_paged_fp8: cln_kv_append_paged with k_scale, v_scale behind seqlens. k_new, v_new, q, q_out are fp16 and rope_table fp32 as there;
 * q is rotated and written as fp16 exactly as there, without a scale. For every element of a live K or V row the kernel stores, all in IEEE fp32:
 *   inv = 1.0f / scale[h];  z = y * inv;  z clamped to [-448, 448];  the byte = z rounded to e4m3 to nearest, ties to even,
 * where y is the fp16 input converted exactly (V, and K with rope_mode 0) or the fp32 rotation result x1 c - x2 s, x1 s + x2 c, with no rounding to
 * fp16 in between. Values beyond 448 scale[h] saturate to +-448 scale[h]; no NaN byte is ever written. A token that is not live writes nothing to
 * the pools and zeros to its q_out rows; a table entry outside [0, P) stores nothing. One launch, no workspace, no atomics.
 * Returns as cln_kv_append_paged, with k_scale, v_scale among the required pointers (4-byte aligned, equal to no output).
 *
 * cln_fa2_decode_paged_fp8: cln_fa2_decode_paged with k_scale, v_scale behind seqlens; q, o fp16 [B,Hq,D], lse fp32 [B,Hq] or NULL:
 *   O[b,h,:] = sum_{j < len_b} softmax_j(q[b,h] . (k8_j k_scale[h / G]) / sqrt(D)) (v8_j v_scale[h / G]),
 * LSE the natural log of the partition sum of those scaled scores. The scales are folded out of the loop (k_scale into the score multiplier,
 * v_scale into the workgroup's partial), so results are bit-repeatable and a sequence's bits depend neither on its neighbours nor on where its
 * pages lie. cln_fa2_decode_paged_fp8_plan: as cln_fa2_decode_paged_plan, with the key step of the FP8 kernel (256 keys at D = 64, 128 at
 * D = 128): *chunk is a multiple of max(page, that step), the workspace formula is the same. The plans of the fp16 and the FP8 entry may differ.
 * Returns as cln_fa2_decode_paged, with k_scale, v_scale among the required 4-byte aligned inputs.
 * The *_describe entries write the kernel instantiation and the launch / plan as text, as their fp16 counterparts do.
 * Not provided: e5m2, per-token or per-page scales, scales computed on the device, FP8 q or o.
 */
int cln_kv_append_paged_fp8(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table, const int* seqlens,
                            const float* k_scale, const float* v_scale, const void* q, void* q_out, const float* rope_table, int B, int T, int Hq,
                            int Hkv, int P, int max_pages, int page, int D, int max_pos, int rope_mode, void* stream);
int cln_kv_append_paged_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode, char* buf, int len);
int cln_fa2_decode_paged_fp8_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                             const float* k_scale, const float* v_scale, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                             int Hq, int Hkv, int P, int max_pages, int page, int D, void* stream);
int cln_fa2_decode_paged_fp8_describe(int B, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);

/* ---- The other two readers of the FP8 cache: multi-token decode (T <= 8) and prefill (any T) attention on the matrix cores.
 * cln_fa2_decode_paged_multi_fp8 is cln_fa2_decode_paged_multi and cln_fa2_prefill_paged_fp8 is cln_fa2_prefill_paged with the pools, the scales
 * and the caller's contract of the section above (k_scale, v_scale behind seqlens): q, o fp16 [B,T,Hq,D], lse fp32 [B,T,Hq] or NULL,
 *   O[b,t,h,:] = sum_{j < n(b,t)} softmax_j(q[b,t,h] . (k8_j k_scale[h / G]) / sqrt(D)) (v8_j v_scale[h / G]),   n(b,t) = len_b - (T - 1 - t),
 * LSE the natural log of the partition sum of those scaled scores, n(b,t) <= 0: O = 0 and LSE = -inf; len_b, the right-aligned ragged batch,
 * D, G, page and the limits as for the fp16 entries. The kernels are the fp16 ones reading bytes: every element is converted to fp16 once
 * (exactly: every e4m3 value is an fp16 value) and both products run on v_mfma_f32_16x16x32_f16 over the unscaled codes; k_scale enters the fp32
 * score multiplier and v_scale the normalisation (the workgroup's partial with a split plan). The pools are inputs and are not written.
 * Deterministic; a sequence's bits depend neither on its neighbours nor on where its pages lie.
 * cln_fa2_decode_paged_multi_fp8_plan: the plan of cln_fa2_decode_paged_multi (the same 128-key step, the same workspace formula), a function of
 * its arguments alone. Returns as the fp16 entries, with k_scale, v_scale among the required inputs (4-byte aligned, equal to no output).
 * The *_describe entries write the kernel instantiation and the plan / grid as text, as their fp16 counterparts do.
 */
int cln_fa2_decode_paged_multi_fp8_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk,
                                        long long* workspace_bytes);
int cln_fa2_decode_paged_multi_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                   const float* k_scale, const float* v_scale, void* o, float* lse, void* workspace, long long workspace_bytes,
                                   int B, int T, int Hq, int Hkv, int P, int max_pages, int page, int D, void* stream);
int cln_fa2_decode_paged_multi_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);
int cln_fa2_prefill_paged_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                              const float* k_scale, const float* v_scale, void* o, float* lse, int B, int T, int Hq, int Hkv, int P, int max_pages,
                              int page, int D, void* stream);
int cln_fa2_prefill_paged_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);

/* ---- The fp16 PAGED KV cache with a PACKED batch: a per-sequence number of new tokens (the cu_seqlens_q convention of varlen attention).
 * cln_fa2_prefill_paged_varlen is cln_fa2_prefill_paged and cln_kv_append_paged_varlen is cln_kv_append_paged with T replaced per sequence by
 * T_b = cu_q[b+1] - cu_q[b]: q, o (k_new, v_new, q_out) are [total_q,H,D], and the tokens of sequence b are the packed rows cu_q[b] .. cu_q[b+1]-1.
 * cu_q: int32 [B+1] ON THE DEVICE and never read by the host, non-decreasing, 0 <= cu_q[0], cu_q[B] <= total_q; both grids are sized from B and
 * total_q alone. len_b = clamp(seqlens[b], 0, max_pages page) counts the T_b newest tokens; token i of sequence b stands at
 * pos = seqlens[b] - T_b + i (64 bits) and sees the keys j < n(b,i) = len_b - (T_b - 1 - i); n <= 0 gives o = 0 and lse = -inf. The append's
 * liveness rule, rotation, pointer rules and q_out zero fill are those of cln_kv_append_paged. T_b = 0 is allowed. PACKED ROWS BELOW cu_q[0] OR AT
 * AND PAST cu_q[B] BELONG TO NO SEQUENCE: neither entry reads or writes them. A cu_q outside this contract gives unspecified values but touches no
 * memory outside the tensors (offsets are clamped to [0, total_q], T_b to >= 0).
 * q, o: fp16 [total_q,Hq,D]; lse: fp32 [total_q,Hq] or NULL; k_new, v_new: fp16 [total_q,Hkv,D]; q, q_out of the append: fp16 [total_q,Hq,D] or both
 * NULL; every other tensor as in the fixed-T entries. Supported: D in {64, 128}; page in {16, 32, 64, 128, 256}; G = Hq / Hkv in {1, 2, 4, 8} for the
 * attention, any multiple for the append; max_pages page < 2^31. One launch each, no workspace, no atomics, deterministic: the attention gives a
 * sequence's tiles of 128 rows r = i G + g from the sequence's own row 0, so its bits are those of cln_fa2_prefill_paged called on that sequence
 * alone with T = T_b, and depend neither on its neighbours nor on its place in the packed tensor.
 * Returns 0, -1 (a NULL or misaligned pointer -- cu_q, block_table, seqlens, lse, rope_table need 4 bytes, the tensors 16; a non-positive B, total_q
 * or other dimension; Hq % Hkv != 0; the pointer rules of rope_mode; forbidden aliasing, q_out == q stays allowed), -2 (other D, G, page or
 * rope_mode; max_pages page >= 2^31; total_q G >= 2^31 or a grid that does not fit) -- all checked before any device access -- or -3 (launch
 * error). The *_describe entries write the kernel, its geometry and the grid as text into buf (at most len bytes, NUL-terminated) and return the
 * text's length, or the same -1 / -2.
 */
int cln_fa2_prefill_paged_varlen(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                 const int* cu_q, void* o, float* lse, int B, int total_q, int Hq, int Hkv, int P, int max_pages,
                                 int page, int D, void* stream);
int cln_fa2_prefill_paged_varlen_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);
int cln_kv_append_paged_varlen(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table,
                               const int* seqlens, const int* cu_q, const void* q, void* q_out, const float* rope_table, int B,
                               int total_q, int Hq, int Hkv, int P, int max_pages, int page, int D, int max_pos, int rope_mode,
                               void* stream);
int cln_kv_append_paged_varlen_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode,
                                        char* buf, int len);

/* ---- The PAGED KV cache in bf16: one full serving step on bf16 tensors -- append with fused RoPE, prefill of a packed
 * batch, multi-token decode. Each entry is its fp16 namesake (cln_kv_append_paged_varlen, cln_fa2_prefill_paged_varlen,
 * cln_fa2_decode_paged_multi[_plan|_describe]) with every fp16 tensor -- q, o, k_new, v_new, q_out, k_pages, v_pages -- in bf16 instead: the same
 * argument lists, shapes, status codes, alignment and aliasing rules, clamping, liveness and n <= 0 -> o = 0, lse = -inf. lse, rope_table and the
 * workspace stay fp32; cln_fa2_decode_paged_multi_bf16_plan returns what cln_fa2_decode_paged_multi_plan returns for the same seven numbers. A fixed
 * T is cu_q = T arange(B + 1).
 * Numerics: K, V and q are bf16 operands of v_mfma_f32_16x16x32_bf16, scores fp32 with the scale log2(e) / sqrt(D) applied to them in fp32; P is
 * rounded once to bf16 (round to nearest even) for the P V product; accumulators, m, l, the split partials and the combine are fp32; o is rounded
 * once to bf16 at the store. The append rotates in fp32 from the bf16 inputs with one rounding to bf16; V rows and rope_mode 0 rows are copied bit
 * for bit. No value passes through fp16: inputs of magnitude 2^17 come through finite.
 */
int cln_kv_append_paged_varlen_bf16(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table,
                                    const int* seqlens, const int* cu_q, const void* q, void* q_out, const float* rope_table, int B,
                                    int total_q, int Hq, int Hkv, int P, int max_pages, int page, int D, int max_pos, int rope_mode,
                                    void* stream);
int cln_kv_append_paged_varlen_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode,
                                             char* buf, int len);
int cln_fa2_prefill_paged_varlen_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                      const int* cu_q, void* o, float* lse, int B, int total_q, int Hq, int Hkv, int P, int max_pages,
                                      int page, int D, void* stream);
int cln_fa2_prefill_paged_varlen_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);
int cln_fa2_decode_paged_multi_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk,
                                         long long* workspace_bytes);
int cln_fa2_decode_paged_multi_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                    void* o, float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P,
                                    int max_pages, int page, int D, void* stream);
int cln_fa2_decode_paged_multi_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len);

/* ---- SLIDING-WINDOW attention over the bf16 paged KV cache: cln_fa2_prefill_paged_varlen_bf16 and
 * cln_fa2_decode_paged_multi_bf16[_plan|_describe] with one more argument, `int window` = W >= 1, behind D. The query token at absolute position
 * p = len_b - T_b + t sees key j iff max(0, p - W + 1) <= j <= p: W keys, its own among them (HF sliding_window = W, FlashAttention
 * window_size = (W - 1, 0)). Everything else is the unwindowed bf16 entry's: tensors, layouts, G, pages, D, alignment and aliasing rules, the
 * clamping of seqlens and cu_q, untouched rows of no sequence, the numerics (fp32 scores scaled in fp32, P rounded once to bf16, fp32 m / l /
 * accumulators, o rounded once at the store, natural-log lse), a row that sees no key -> o = 0, lse = -inf, no host read of device data,
 * deterministic. With W >= max_pages page the results are bit for bit those of the unwindowed entries.
 * Plan: cln_fa2_decode_paged_multi_window_bf16_plan divides not max_pages page but span = min(max_pages page, round_up(W + T - 1, U) + U) keys,
 * U = max(page, 128), into `splits` chunks of `chunk` keys counted from base_b = align_down(max(0, len_b - T - W + 1), U) of each sequence; a
 * function of its eight numbers only, and for W >= max_pages page the plan of cln_fa2_decode_paged_multi_bf16_plan. The workspace layout and size
 * rule are unchanged.
 * Stale table entries: with lo_min_b = max(0, len_b - T_b - W + 1), neither entry reads a block-table entry, or a pool row, of a logical page
 * that ends at or before align_down(lo_min_b, U), U = max(page, 64) for the prefill and max(page, 128) for the decode: the caller may free or
 * reuse those pages, and the table entries may be stale (any value).
 * Returns the unwindowed entry's status for the same arguments, and -1 for window <= 0 (checked behind the shape).
 */
int cln_fa2_prefill_paged_varlen_window_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                             const int* seqlens, const int* cu_q, void* o, float* lse, int B, int total_q, int Hq, int Hkv, int P,
                                             int max_pages, int page, int D, int window, void* stream);
int cln_fa2_prefill_paged_varlen_window_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int window, char* buf,
                                                      int len);
int cln_fa2_decode_paged_multi_window_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, int* splits,
                                                int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_multi_window_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                           void* o, float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P,
                                           int max_pages, int page, int D, int window, void* stream);
int cln_fa2_decode_paged_multi_window_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, char* buf,
                                                    int len);

/* ---- ATTENTION SINKS on the sliding-window bf16 paged entries: the *_window_bf16 entries above with one more input,
 * `const float* sinks` = fp32 [Hq] on the device, the last input pointer: behind cu_q for the prefill, behind seqlens for the decode. sinks[h] is
 * one logit per query head in natural-log units, as the model stores it (cast to fp32 by the caller) and NOT multiplied by 1/sqrt(D); it takes
 * part in the softmax denominator of every row of head h and contributes no value (HF GptOssAttention: a sink column concatenated to the scaled
 * logits, softmax, the column dropped).
 * Mask: position, causal edge, window, ragged and right-aligned batches, len_b < T_b, the clamping of seqlens and cu_q, stale table entries and
 * the rows of no sequence are exactly those of the *_window_bf16 entries. A window past the cache (any W >= max_pages page, e.g. 2^31 - 1) is
 * full causal attention with sinks.
 * A row that sees at least one key, with s_j = q.k_j / sqrt(D) over its visible keys j:
 *   o   = sum_j exp(s_j) v_j / (sum_j exp(s_j) + exp(sinks[h]))
 *   lse = ln(sum_j exp(s_j) + exp(sinks[h])): the log of the denominator ACTUALLY USED, the sink included -- not the log-sum-exp over the keys.
 * Evaluated without overflow for every sink whose sink log2(e) is finite in fp32: with m, l the row's fp32 maximum and sum in log2 units,
 * m' = max(m, sink2), o and l are scaled by exp2(m - m') and exp2(sink2 - m') is added to l; sink2 = sinks[h] log2(e) is formed once, in fp32.
 * A row that sees no key (a right-aligned padding row, len_b = 0, len_b < T_b): o = 0, lse = -inf, as in the *_window_bf16 entries; the sink
 * does not turn a non-row into a row.
 * The sink enters once per row whatever the number of splits: at the final normalisation of the prefill kernel and of the decode's stream kernel
 * when splits == 1, in the combine kernel when splits > 1 (the splits store raw partials; the workspace layout is unchanged).
 * sinks[h] = -inf, or a finite sink so far below the row's maximum that exp2 gives 0: o and lse are bit for bit those of the *_window_bf16 entry.
 * Plan: cln_fa2_decode_paged_multi_window_sink_bf16_plan is cln_fa2_decode_paged_multi_window_bf16_plan; the sink changes neither the splits nor
 * the workspace.
 * sinks is required (without sinks use the *_window_bf16 entry), 4-byte aligned and no output. Returns the *_window_bf16 entry's status for the
 * same arguments in the same order; a null or misaligned sinks, or sinks equal to o, lse or workspace, is -1 where a bad seqlens is.
 */
int cln_fa2_prefill_paged_varlen_window_sink_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                  const int* seqlens, const int* cu_q, const float* sinks, void* o, float* lse, int B, int total_q,
                                                  int Hq, int Hkv, int P, int max_pages, int page, int D, int window, void* stream);
int cln_fa2_prefill_paged_varlen_window_sink_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                           char* buf, int len);
int cln_fa2_decode_paged_multi_window_sink_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, int* splits,
                                                     int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_multi_window_sink_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                const int* seqlens, const float* sinks, void* o, float* lse, void* workspace,
                                                long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages, int page, int D,
                                                int window, void* stream);
int cln_fa2_decode_paged_multi_window_sink_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, char* buf,
                                                         int len);

/* ---- FP8 (OCP e4m3fn) KV POOLS on the bf16 paged path, with window and sinks: a bf16 model keeps its cache in one
 * byte per element. Three entries, the most general form -- a full-attention layer passes a window past the cache, a layer without sinks passes
 * sinks = NULL. k_pages / v_pages are e4m3fn [P,Hkv,page,D]; k_scale / v_scale are fp32 [Hkv] on the device, finite and > 0, with the meaning and
 * the rules of the fp16 FP8 entries (section 14): a stored byte c of KV head h means e4m3(c) * scale[h], and the live bytes are no NaN code
 * (0x7f, 0xff). q, o, k_new, v_new and q_out are bf16. The scales stand behind cu_q (append, prefill) or seqlens (decode), 4-byte aligned.
 *
 * cln_kv_append_paged_varlen_bf16_fp8: cln_kv_append_paged_varlen_bf16 with the quantising store of cln_kv_append_paged_fp8 -- the packed cu_q
 * prologue, liveness, clamping, the rows of no sequence left untouched, q -> q_out rotated and stored as bf16 (q_out == q allowed). Per element of
 * a live K or V row the byte is e4m3(clamp(y * (1.0f / scale[h]), -448, 448)), IEEE fp32, round to nearest even, y the bf16 input or the fp32
 * rotation result with no bf16 rounding in between. Status: that of cln_kv_append_paged_varlen_bf16 for the same arguments; a null or misaligned
 * scale, or a scale that is an output, is -1 where a bad cu_q is.
 *
 * cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8 / cln_fa2_decode_paged_multi_window_sink_bf16_fp8: the function of the *_window_sink_bf16
 * entries above evaluated on the dequantised pools -- position, causal edge, window max(0, p - W + 1) <= j <= p, ragged and right-aligned
 * batches, len_b < T_b, stale table entries (the same U), rows that see no key (o = 0, lse = -inf) and lse = the log of the denominator used are
 * theirs. Any window >= max_pages page means no window. sinks may be NULL: no sink, bit for bit the result of a [Hq] tensor of -inf.
 * Numerics: every code is converted once to bf16, exactly (v_cvt_scalef32_pk_bf16_fp8 at scale 2^0; every e4m3 value is a bf16 value); both
 * products run on v_mfma_f32_16x16x32_bf16 on the unscaled codes; k_scale[kvh] log2(e) / sqrt(D) is the fp32 score multiplier, one product per
 * workgroup; v_scale[kvh] multiplies the prefill's normalisation, respectively the decode's fp32 partial in front of its store. P is rounded
 * once to bf16 (round to nearest even); m, l, accumulators, partials and the combine are fp32; o is rounded once to bf16 at the store. Nothing
 * passes through fp16.
 * Plan: cln_fa2_decode_paged_multi_window_sink_bf16_fp8_plan is cln_fa2_decode_paged_multi_window_bf16_plan, status included; the workspace is
 * fp32 and has the same layout, and the splits are merged by the *_window_sink_bf16 entry's combine kernel (without sinks: the *_window_bf16
 * entry's).
 * Status: that of the *_window_sink_bf16 entry for the same arguments in the same order, except that sinks == NULL is legal (a misaligned sinks,
 * or sinks equal to an output, stays -1); a null or misaligned scale, or a scale equal to an output, is -1 where a bad seqlens is; window <= 0 is
 * -1, checked behind the shape. D in {64, 128}, Hq / Hkv in {1, 2, 4, 8}, page in {16, 32, 64, 128, 256}, T <= 8 for the decode.
 */
int cln_kv_append_paged_varlen_bf16_fp8(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table,
                                        const int* seqlens, const int* cu_q, const float* k_scale, const float* v_scale, const void* q,
                                        void* q_out, const float* rope_table, int B, int total_q, int Hq, int Hkv, int P, int max_pages, int page,
                                        int D, int max_pos, int rope_mode, void* stream);
int cln_kv_append_paged_varlen_bf16_fp8_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode, char* buf,
                                                 int len);
int cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                      const int* seqlens, const int* cu_q, const float* k_scale, const float* v_scale,
                                                      const float* sinks /* may be NULL */, void* o, float* lse, int B, int total_q, int Hq,
                                                      int Hkv, int P, int max_pages, int page, int D, int window, void* stream);
int cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                               char* buf, int len);
int cln_fa2_decode_paged_multi_window_sink_bf16_fp8_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, int* splits,
                                                         int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_multi_window_sink_bf16_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                    const int* seqlens, const float* k_scale, const float* v_scale,
                                                    const float* sinks /* may be NULL */, void* o, float* lse, void* workspace,
                                                    long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages, int page,
                                                    int D, int window, void* stream);
int cln_fa2_decode_paged_multi_window_sink_bf16_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, char* buf,
                                                             int len);

/* ---- ANY QUERY-GROUP SIZE G = Hq / Hkv in 1 ... 16 on the bf16 paged attention path: the entries above take
 * G in {1, 2, 4, 8} only and keep doing so; these four take every integer G from 1 to 16 -- 3 (Llama-3.2-3B), 5, 6, 7 (Qwen2.5), 12, 16
 * (Llama-3.1-405B, Qwen3-235B) among them. The append entries take any Hq % Hkv == 0 as they are. Each is the most general form: a
 * full-attention layer passes a window past the cache, a layer without sinks passes sinks = NULL (legal in all four, the bf16 pair included: bit
 * for bit the result of a [Hq] tensor of -inf).
 *
 * cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16 / cln_fa2_decode_paged_multi_window_sink_anyg_bf16: the function, the tensors and the
 * argument list of the *_window_sink_bf16 entries (section 19). *_anyg_bf16_fp8: those of the *_window_sink_bf16_fp8 entries (section 20). Query
 * head h reads KV head h / G (integer division); row r = t G + g of a (sequence, KV head) is token t = r / G, head kvh G + g. The kernels divide
 * (unsigned 32-bit, exact for every row) in front of and behind the key loop, which is the sibling's, statement for statement. For G in
 * {1, 2, 4, 8}, o and lse are the sibling's bit for bit.
 * Decode: a workgroup serves the T G rows of a (sequence, KV head) in ceil(T G / 16) <= 4 row tiles, so T <= 8 AND T G <= 64: G = 16 with
 * T <= 4, G = 12 with T <= 5, G <= 8 with any T <= 8. The prefill has no such limit.
 * Plan: fa2d::split_plan of (B Hkv, B T Hq, the window entry's span and unit, D) -- for G in {1, 2, 4, 8} cln_fa2_decode_paged_multi_window_bf16_plan,
 * status included. The workspace is fp32 in the siblings' layout; the splits are merged by the siblings' combine kernels.
 * Status: that of the sibling for the same arguments in the same order, except: Hq / Hkv in 1 ... 16 is legal and G > 16 is -2; the decode's
 * T G > 64 is -2 where T > 8 is; sinks == NULL is legal (a misaligned sinks, or sinks equal to an output, stays -1). Hq % Hkv != 0 is -1;
 * window <= 0 is -1, checked behind the shape. D in {64, 128}, page in {16, 32, 64, 128, 256}.
 */
int cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                       const int* seqlens, const int* cu_q, const float* sinks /* may be NULL */, void* o,
                                                       float* lse, int B, int total_q, int Hq, int Hkv, int P, int max_pages, int page, int D,
                                                       int window, void* stream);
int cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                char* buf, int len);
int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, int* splits,
                                                          int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_multi_window_sink_anyg_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                     const int* seqlens, const float* sinks /* may be NULL */, void* o, float* lse,
                                                     void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P,
                                                     int max_pages, int page, int D, int window, void* stream);
int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, char* buf,
                                                              int len);
int cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                           const int* seqlens, const int* cu_q, const float* k_scale, const float* v_scale,
                                                           const float* sinks /* may be NULL */, void* o, float* lse, int B, int total_q, int Hq,
                                                           int Hkv, int P, int max_pages, int page, int D, int window, void* stream);
int cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D,
                                                                    int window, char* buf, int len);
int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                              int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                         const int* seqlens, const float* k_scale, const float* v_scale,
                                                         const float* sinks /* may be NULL */, void* o, float* lse, void* workspace,
                                                         long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages, int page,
                                                         int D, int window, void* stream);
int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                  char* buf, int len);

/* ---- SOFTMAX SCALE AND LOGIT SOFT-CAPPING on the bf16 paged attention path: the entries above fix the softmax scale
 * at 1 / sqrt(D) and have no soft-capping, and keep doing so; these four are the any-G entries with two floats behind `window`. Gemma-2-27B
 * (D = 128, query_pre_attn_scalar 144, cap 50), Gemma-3-27B (168, no cap), Granite (attention_multiplier) and Grok-1 (G = 6, cap 30) need them.
 *
 * With x = softmax_scale, or 1 / sqrt(D) when softmax_scale == 0, a row of head h that sees the keys lo <= j < n has u_j = q.k_j x and
 *   s_j = u_j                        softcap == 0: no cap
 *   s_j = softcap tanh(u_j / softcap)  otherwise
 *   O = sum_j exp(s_j) v_j / (sum_j exp(s_j) + exp(sink_h)),  LSE = ln of that denominator.
 * The sink is neither scaled nor capped. The window and causal mask are applied after the cap: a hidden key is -inf, not -softcap. A row that
 * sees no key stays O = 0, LSE = -inf. FP8 pools: k_scale[kv head] is part of the dequantised score and stands inside the tanh; v_scale stays in
 * the normalisation.
 * softmax_scale: 0 means 1 / sqrt(D), with the multiplier the any-G entries pass; any other value is finite and > 0 and the score multiplier is
 * (float)((double)softmax_scale log2(e)). softcap: 0 means no cap, and the kernel that runs is the any-G body; any other value is finite and > 0.
 * With both 0, o and lse are the any-G entries' bit for bit. A negative, NaN or infinite value of either is -1, checked before anything else --
 * no pointer is looked at. Every other argument, check and status code is the any-G entry's, in its order. The _describe entries take both floats
 * and check them the same way; the _plan entries take neither: the plan of the any-G entry for the same numbers.
 */
int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                               const int* seqlens, const int* cu_q, const float* sinks /* may be NULL */, void* o,
                                                               float* lse, int B, int total_q, int Hq, int Hkv, int P, int max_pages, int page,
                                                               int D, int window, float softmax_scale, float softcap, void* stream);
int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D,
                                                                        int window, float softmax_scale, float softcap, char* buf, int len);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                  int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                             const int* seqlens, const float* sinks /* may be NULL */, void* o, float* lse,
                                                             void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P,
                                                             int max_pages, int page, int D, int window, float softmax_scale, float softcap,
                                                             void* stream);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                      float softmax_scale, float softcap, char* buf, int len);
int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                                   const int* seqlens, const int* cu_q, const float* k_scale,
                                                                   const float* v_scale, const float* sinks /* may be NULL */, void* o, float* lse,
                                                                   int B, int total_q, int Hq, int Hkv, int P, int max_pages, int page, int D,
                                                                   int window, float softmax_scale, float softcap, void* stream);
int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D,
                                                                            int window, float softmax_scale, float softcap, char* buf, int len);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                      int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                                 const int* seqlens, const float* k_scale, const float* v_scale,
                                                                 const float* sinks /* may be NULL */, void* o, float* lse, void* workspace,
                                                                 long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages,
                                                                 int page, int D, int window, float softmax_scale, float softcap, void* stream);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D,
                                                                          int window, float softmax_scale, float softcap, char* buf, int len);

/* ---- HEAD DIM 256 on the bf16 paged path: the entries above take D = 64 and 128 and keep refusing every other head
 * dim with -2; these seven are siblings that take D = 256 and nothing else (-2 for 64, 128, 96 ...). Gemma-2 (2B, 9B: cap 50, W 4096) and
 * Gemma-3 (1B, 4B, 12B: W 512 / 1024) have D = 256.
 *
 * cln_kv_append_paged_varlen_d256_bf16: cln_kv_append_paged_varlen_bf16 on pools bf16 [P,Hkv,page,256]; all three rope modes, the half-split
 * pairs are (i, i + 128). Arguments, checks and status codes are that entry's, in its order.
 * cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16: cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16 at D = 256, the
 * same semantics: cap before the mask, the sink neither scaled nor capped, a row that sees no key O = 0 and LSE = -inf, no page and no table
 * entry wholly below the window read. Arguments, checks and status codes are that entry's, in its order (the two floats first).
 * cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16: cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16 at D = 256 for T in
 * 1 ... 8, G in 1 ... 16 and T G <= 32 (more: -2). Its _plan is its own -- the kernel's key step is 64, not 128, so the chunk is a multiple of
 * max(page, 64) -- and the workspace is sized from it: rows S (256 + 2) 4 bytes when S > 1. Arguments, checks and status codes are that
 * entry's, in its order.
 * Scores and accumulators fp32, both products on v_mfma_f32_16x16x32_bf16, P and O rounded once to bf16; nothing passes through fp16.
 */
int cln_kv_append_paged_varlen_d256_bf16(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table,
                                         const int* seqlens, const int* cu_q, const void* q, void* q_out, const float* rope_table, int B,
                                         int total_q, int Hq, int Hkv, int P, int max_pages, int page, int D, int max_pos, int rope_mode,
                                         void* stream);
int cln_kv_append_paged_varlen_d256_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode, char* buf,
                                                  int len);
int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16(const void* q, const void* k_pages, const void* v_pages,
                                                                    const int* block_table, const int* seqlens, const int* cu_q,
                                                                    const float* sinks /* may be NULL */, void* o, float* lse, int B, int total_q,
                                                                    int Hq, int Hkv, int P, int max_pages, int page, int D, int window,
                                                                    float softmax_scale, float softcap, void* stream);
int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D,
                                                                             int window, float softmax_scale, float softcap, char* buf, int len);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                       int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                                  const int* seqlens, const float* sinks /* may be NULL */, void* o, float* lse,
                                                                  void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P,
                                                                  int max_pages, int page, int D, int window, float softmax_scale, float softcap,
                                                                  void* stream);
int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D,
                                                                           int window, float softmax_scale, float softcap, char* buf, int len);

/* ---- MULTI-HEAD LATENT ATTENTION (MLA) over a paged latent cache, bf16: the cache of DeepSeek-V2 / V3 / R1 and
 * Kimi-K2. One pool bf16 [P, page, 576] of latent rows [c (512) | k_pe (64)], stored once and shared by every query head: the same row is the
 * key (all 576 dims) and the value (dims 0 ... 511); Hkv = 1 by construction. page a power of two in 16 ... 256, block_table int32
 * [B, max_pages], seqlens int32 [B] on the device, counting the new tokens, max_pages page < 2^31.
 *
 * cln_fa2_decode_paged_mla_bf16: q bf16 [B,T,Hq,576], already absorbed by the model (q_nope W_UK in dims 0 ... 511, q_pe in 512 ... 575); o bf16
 * [B,T,Hq,512] in latent space (the model applies W_UV); lse fp32 [B,T,Hq], natural log, or NULL. Query (b, t, h) sees the keys
 * j < len_b - (T - 1 - t); s_j = softmax_scale q . row_j[0:576]; O = softmax(s) row[:, 0:512], rounded once; a row that sees no key gets O = 0 and
 * LSE = -inf. softmax_scale is required, finite and > 0 (the models use 192^-1/2 mscale^2): anything else is -1, checked first. T in 1 ... 8, Hq in
 * 1 ... 128 (more: -2), any R = T Hq; rows are ordered r = t Hq + h. No window, no sinks, no cap. The workspace is that of _plan,
 * B T Hq S (512 + 2) 4 bytes when S > 1; the plan is a function of the shape only: fa2d::split_plan on B ceil(T Hq / 64) workgroup jobs in units of
 * max(page, 64) keys. Statuses as the siblings': -1 for a bad argument, -2 for unsupported. Every pool row is fetched from global memory once per
 * workgroup and serves both products, on v_mfma_f32_16x16x32_bf16 with fp32 scores and accumulators; nothing passes through fp16.
 * cln_kv_append_paged_mla_bf16: a packed batch in the cu_q convention of cln_kv_append_paged_varlen_bf16. c_new bf16 [total_q,512] goes to pool
 * dims 0 ... 511 bit for bit, k_pe_new bf16 [total_q,64] to dims 512 ... 575, rotated at the token's position seqlens[b] - T_b + i; q / q_out bf16
 * [total_q,Hq,576] or both NULL (q_out may be q): dims 0 ... 511 copied bit for bit, dims 512 ... 575 rotated at the same position. rope_table fp32
 * [max_pos,64] = [cos 32 | sin 32]; rope_mode 0 none (no table; the rotary dims are copied), 1 half-split pairs (i, i + 32), 2 interleaved. The
 * rotation is the bf16 append's: fp32 from the bf16 inputs, one rounding. One launch, nothing read on the host, rows of no sequence untouched.
 */
int cln_fa2_decode_paged_mla_bf16_plan(int B, int T, int Hq, int max_pages, int page, int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_mla_bf16(const void* q, const void* pool, const int* block_table, const int* seqlens, void* o, float* lse,
                                  void* workspace, long long workspace_bytes, int B, int T, int Hq, int P, int max_pages, int page,
                                  float softmax_scale, void* stream);
int cln_fa2_decode_paged_mla_bf16_describe(int B, int T, int Hq, int max_pages, int page, float softmax_scale, char* buf, int len);
int cln_kv_append_paged_mla_bf16(const void* c_new, const void* k_pe_new, void* pool, const int* block_table, const int* seqlens,
                                 const int* cu_q, const void* q, void* q_out, const float* rope_table, int B, int total_q, int Hq, int P,
                                 int max_pages, int page, int max_pos, int rope_mode, void* stream);
int cln_kv_append_paged_mla_bf16_describe(int B, int total_q, int Hq, int max_pages, int page, int rope_mode, char* buf, int len);

/* ---- MLA PREFILL (un-absorbed), the merge of two attention states and the gather out of the latent pool, bf16:
 * the prompt path in front of the two entries above. For a prompt these models up-project the latent rows with kv_b_proj and run ordinary
 * attention per head with a key of 192 dims (128 "nope" + 64 rotary) and a value of 128, Hkv = Hq.
 *
 * cln_fa2_prefill_varlen_mla_bf16: a packed batch. q bf16 [total_q,Hq,192] = [q_nope 128 | q_pe 64], already rotated; kv bf16 [total_k,Hq,256] =
 * [k_nope 128 | v 128] per head, exactly what kv_b_proj writes; k_pe bf16 [total_k,64], rotated, one row per token shared by every head (never
 * broadcast in memory); cu_q, cu_k int32 [B+1] on the device, never read by the host, every offset clamped to [0, total_q] / [0, total_k],
 * T_b = max(cu_q[b+1] - cu_q[b], 0), L_b likewise from cu_k; o bf16 [total_q,Hq,128]; lse fp32 [total_q,Hq], natural log, or NULL. causal = 1:
 * query t of sequence b sees the keys j < L_b - (T_b - 1 - t); causal = 0: all L_b keys (a context chunk of a chunked prefill). A query that sees
 * no key gets O = 0 and LSE = -inf. softmax_scale is required, finite and > 0: anything else is -1, checked first. Then -1 for a missing,
 * misaligned (q, kv, k_pe, o 16 bytes; cu_q, cu_k, lse 4) or aliased pointer or a non-positive B, total_q, total_k or Hq; -2 for Hq > 128, a causal
 * that is neither 0 nor 1, or a grid that does not fit. Packed rows outside [cu_q[0], cu_q[B]) are neither read nor written. No pages, window,
 * sinks or cap. One launch, no workspace, Hq (total_q / 128 + B) workgroups; v_mfma_f32_16x16x32_bf16 with fp32 scores and accumulators, nothing
 * passes through fp16; deterministic.
 * cln_attn_merge_states_bf16: joins two attention states over disjoint key sets. o_a, o_b bf16 [rows,D], lse_a, lse_b fp32 [rows], o bf16
 * [rows,D] (may be o_a), lse fp32 [rows] or NULL (may be lse_a); D % 8 == 0, 8 <= D <= 512 (else -2). Per row in fp32: m = max(lse_a, lse_b);
 * m = -inf: O = 0, LSE = -inf; else w = exp(lse - m) per side, a side whose LSE is -inf selected out (its O may hold anything, NaN included),
 * O = (w_a O_a + w_b O_b) / (w_a + w_b) rounded once to bf16, LSE = m + ln(w_a + w_b). One launch, deterministic.
 * cln_kv_gather_paged_mla_bf16: pool bf16 [P,page,576], block_table int32 [B,max_pages], starts int32 [B] or NULL (0), cu_k int32 [B+1], out bf16
 * [total_k,576]. Packed row cu_k[b] + i receives cache row starts[b] + i of sequence b for i < cu_k[b+1] - cu_k[b], bit for bit; a cache row at
 * or past max_pages page is written as zeros and its table entry never followed; rows of no sequence are untouched. The mirror of
 * cln_kv_append_paged_mla_bf16, with its statuses.
 */
int cln_fa2_prefill_varlen_mla_bf16(const void* q, const void* kv, const void* k_pe, const int* cu_q, const int* cu_k, void* o, float* lse, int B,
                                    int total_q, int total_k, int Hq, int causal, float softmax_scale, void* stream);
int cln_fa2_prefill_varlen_mla_bf16_describe(int B, int total_q, int total_k, int Hq, int causal, float softmax_scale, char* buf, int len);
int cln_attn_merge_states_bf16(const void* o_a, const float* lse_a, const void* o_b, const float* lse_b, void* o, float* lse, long long rows,
                               int D, void* stream);
int cln_attn_merge_states_bf16_describe(long long rows, int D, char* buf, int len);
int cln_kv_gather_paged_mla_bf16(const void* pool, const int* block_table, const int* starts, const int* cu_k, void* out, int B, int total_k,
                                 int P, int max_pages, int page, void* stream);
int cln_kv_gather_paged_mla_bf16_describe(int B, int total_k, int max_pages, int page, char* buf, int len);

/* ---- MLA over a paged latent cache held in FP8 (OCP e4m3fn), bf16 queries: the three entries above that touch the
 * pool, on a pool of codes. pool [P, page, 576] of bytes, a row [c (512) | k_pe (64)] in codes, 576 bytes; kv_scale fp32 [1] ON THE DEVICE, one
 * scale for the whole row: value = e4m3(code) kv_scale. The caller guarantees a finite kv_scale > 0 and no NaN code (0x7f, 0xff) in a live row;
 * the kernels do not check either. block_table, seqlens, cu_q, cu_k, starts, the page sizes and max_pages page < 2^31 are the bf16 entries'; q,
 * q_out, c_new, k_pe_new, o and the gather's out stay bf16. Arguments, checks and status codes are the bf16 entries', in their order; kv_scale
 * stands behind seqlens (append: cu_q, gather: cu_k) and a missing one, one not 4-byte aligned or one equal to an output is -1 there, before
 * the shape. The decode's softmax_scale check stays first.
 *
 * cln_kv_append_paged_mla_bf16_fp8: cln_kv_append_paged_mla_bf16 with a quantising store. Per element of a live pool row, in fp32:
 * byte = e4m3(clamp(y (1.0f / kv_scale), +-448)), round to nearest even, y the bf16 input or the fp32 rotation result with no bf16 rounding in
 * between. q / q_out as there, bf16.
 * cln_fa2_decode_paged_mla_bf16_fp8: cln_fa2_decode_paged_mla_bf16 on the dequantised pool. The codes are converted to bf16 exactly on the way
 * to LDS, once per workgroup; the fp32 score multiplier is (softmax_scale log2 e) kv_scale and kv_scale multiplies the fp32 result in front of
 * its store, so the partials of a split carry it. _plan returns what cln_fa2_decode_paged_mla_bf16_plan returns, status included.
 * cln_kv_gather_paged_mla_bf16_fp8: cln_kv_gather_paged_mla_bf16 with a dequantising load; an element of out is bf16(fp32(code) kv_scale), one
 * rounding.
 */
int cln_kv_append_paged_mla_bf16_fp8(const void* c_new, const void* k_pe_new, void* pool, const int* block_table, const int* seqlens,
                                     const int* cu_q, const float* kv_scale, const void* q, void* q_out, const float* rope_table, int B,
                                     int total_q, int Hq, int P, int max_pages, int page, int max_pos, int rope_mode, void* stream);
int cln_kv_append_paged_mla_bf16_fp8_describe(int B, int total_q, int Hq, int max_pages, int page, int rope_mode, char* buf, int len);
int cln_fa2_decode_paged_mla_bf16_fp8_plan(int B, int T, int Hq, int max_pages, int page, int* splits, int* chunk, long long* workspace_bytes);
int cln_fa2_decode_paged_mla_bf16_fp8(const void* q, const void* pool, const int* block_table, const int* seqlens, const float* kv_scale, void* o,
                                      float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq, int P, int max_pages,
                                      int page, float softmax_scale, void* stream);
int cln_fa2_decode_paged_mla_bf16_fp8_describe(int B, int T, int Hq, int max_pages, int page, float softmax_scale, char* buf, int len);
int cln_kv_gather_paged_mla_bf16_fp8(const void* pool, const int* block_table, const int* starts, const int* cu_k, const float* kv_scale,
                                     void* out, int B, int total_k, int P, int max_pages, int page, void* stream);
int cln_kv_gather_paged_mla_bf16_fp8_describe(int B, int total_k, int max_pages, int page, char* buf, int len);

/* ---- Sparse MLA decode over the paged latent cache, bf16: DeepSeek-V3.2's attention ("DSA") behind its indexer.
 * q [B,T,Hq,576], pool [P,page,576], block_table [B,max_pages], seqlens [B], o [B,T,Hq,512], lse fp32 [B,T,Hq] or null, softmax_scale
 * (required, finite, > 0) are cln_fa2_decode_paged_mla_bf16's. indices int32 [B,T,topk], contiguous, ON THE DEVICE, 4-byte aligned, never read
 * by the host: slot k of indices[b,t] is a LOGICAL token position of sequence b (the position space of seqlens), resolved through the block
 * table, the same list for all heads of the token. A slot is VALID iff 0 <= idx < vis(b,t) = clamp(seqlens[b], 0, max_pages page) - (T - 1 - t),
 * the dense entry's causal edge; every other value -- -1, any negative, anything at or past vis or past the cache -- is an EMPTY slot, may
 * stand anywhere in the list, and addresses no table entry and no pool row. With V the valid slots of a query token all its heads compute
 * s_k = softmax_scale q . row(idx_k)[0:576], O = softmax_V(s) row[:, 0:512], LSE = ln sum_V exp(s_k); V empty: O = 0, LSE = -inf exactly. A
 * position listed twice is two keys: pass distinct positions. Hq in 1 ... 128; topk >= 1, any value; T >= 1 WITHOUT the cap of 8 (a query
 * token is its own workgroup job: the entry is V3.2's sparse prefill over the paged cache too).
 * Status, in this order: the scale (-1); a missing or misaligned pointer (q, pool, o, lse, workspace 16 bytes; block_table, seqlens, indices
 * 4 bytes) or an output equal to an input or another output (-1); P <= 0 (-1); the plan -- a non-positive B, T, Hq, topk, max_pages or page
 * (-1), Hq > 128, another page, max_pages page >= 2^31, B T Hq >= 2^31 or a grid that does not fit (-2); a workspace smaller than the plan's
 * (-1). _plan: a function of the shape only; the splits divide the topk index slots (chunk a multiple of 64), workspace_bytes =
 * B T Hq splits (512 + 2) 4 when splits > 1, else 0. Every split of a row is written and all are merged in ascending order: deterministic.
 */
int cln_fa2_decode_paged_mla_sparse_bf16_plan(int B, int T, int Hq, int topk, int max_pages, int page, int* splits, int* chunk,
                                              long long* workspace_bytes);
int cln_fa2_decode_paged_mla_sparse_bf16(const void* q, const void* pool, const int* block_table, const int* seqlens, const int* indices, void* o,
                                         float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq, int topk, int P,
                                         int max_pages, int page, float softmax_scale, void* stream);
int cln_fa2_decode_paged_mla_sparse_bf16_describe(int B, int T, int Hq, int topk, int max_pages, int page, float softmax_scale, char* buf,
                                                  int len);

/* ---- The indexer of DeepSeek-V3.2's sparse attention ("DSA"), bf16: what produces the `indices` of the entry
 * above. Per layer the model keeps one INDEX KEY of 128 dims per cached token, shared by all index heads: idx_pool bf16 [P,page,128] behind
 * the block table [B,max_pages] and the lengths [B] of the latent cache. Device pointers are never read by the host; every call is one
 * launch, deterministic, capturable, without a workspace.
 *
 * cln_kv_append_paged_index_bf16: k_idx_new bf16 [total_q,128] packed by cu_q int32 [B+1]; the packed convention, seqlens AFTER the append,
 * liveness and the caller's contract are cln_kv_append_paged_mla_bf16's: token i of sequence b is packed row cu_q[b] + i at pos =
 * seqlens[b] - T_b + i, copied bit for bit. No rotation argument, on purpose: the model rotates the key and THEN applies a Hadamard
 * transform before caching. Status: a missing or misaligned pointer (k_idx_new, idx_pool 16 bytes; the int arrays 4) or idx_pool equal to an
 * input (-1); P <= 0 (-1); a non-positive B, total_q, max_pages or page (-1); another page or max_pages page >= 2^31 (-2).
 *
 * cln_mla_index_logits_paged_bf16: q_idx bf16 [B,T,Hi,128], weights fp32 [B,T,Hi] (the caller folds Hi^-1/2, 128^-1/2 and anything else into
 * them), logits fp32 [B,T,ld] contiguous, ld >= 1 the caller's. With cap = min(max_pages page, ld) and vis(b,t) = clamp(seqlens[b], 0, cap) -
 * (T - 1 - t) it writes logits[b,t,j] = sum_h weights[b,t,h] max(0, q_idx[b,t,h] . k_idx[j]) for 0 <= j < vis(b,t) and NOTHING ELSE: a
 * position at or past vis keeps its bytes, and neither its key nor its table entry is read. Any T >= 1, Hi in 1 ... 64. The products run on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation; ReLU, weight and head sum are fp32 in a fixed order that depends on neither the grid, the
 * batch nor the length. Inputs whose dot products are finite give no NaN. Status, in this order: a missing or misaligned pointer (q_idx,
 * idx_pool 16 bytes; weights, block_table, seqlens, logits 4 bytes) or logits equal to an input (-1); P <= 0 (-1); a non-positive B, T, Hi,
 * ld, max_pages or page (-1); Hi > 64, another page, max_pages page >= 2^31, B T >= 2^31 or a grid that does not fit (-2).
 *
 * cln_mla_index_topk: logits as above, indices int32 [B,T,topk] contiguous, any topk >= 1; cap = ld. With n = max(vis(b,t), 0): n <= topk
 * gives indices[b,t] = [0, 1, ..., n - 1, -1, ..., -1] (the dense list: the sparse decode then gives the dense entry's bits); otherwise the
 * topk positions that come first under the total order (logit descending, position ascending), WRITTEN IN ASCENDING POSITION ORDER. Every
 * slot is written on every call; only logits[b,t,0 ... n - 1] is read. The logit order is fp32's numeric order with -0 taken as +0 and +-inf
 * ordinary values; a NaN is ordered by its bit pattern under the map "sign bit set: complement, else set the sign bit"; whatever the values,
 * every written index is -1 or a distinct position in [0, n). Status: a missing or misaligned pointer (4 bytes each) or indices equal to an
 * input (-1); a non-positive B, T, ld or topk (-1); ld >= 2^31, B T >= 2^31, topk B T past 2^61 or a grid that does not fit (B T 1024 >=
 * 2^32) (-2).
 */
int cln_kv_append_paged_index_bf16(const void* k_idx_new, void* idx_pool, const int* block_table, const int* seqlens, const int* cu_q, int B,
                                   int total_q, int P, int max_pages, int page, void* stream);
int cln_kv_append_paged_index_bf16_describe(int B, int total_q, int max_pages, int page, char* buf, int len);
int cln_mla_index_logits_paged_bf16(const void* q_idx, const float* weights, const void* idx_pool, const int* block_table, const int* seqlens,
                                    float* logits, int B, int T, int Hi, long long ld, int P, int max_pages, int page, void* stream);
int cln_mla_index_logits_paged_bf16_describe(int B, int T, int Hi, long long ld, int max_pages, int page, char* buf, int len);
int cln_mla_index_topk(const float* logits, const int* seqlens, int* indices, int B, int T, long long ld, int topk, void* stream);
int cln_mla_index_topk_describe(int B, int T, long long ld, int topk, char* buf, int len);

/* ---- Sparse MLA decode over the paged latent cache held in FP8 (OCP e4m3fn), bf16 queries: the attention of a
 * DeepSeek-V3.2 step on the pool cln_kv_append_paged_mla_bf16_fp8 writes. Semantics are exactly cln_fa2_decode_paged_mla_sparse_bf16's -- a
 * slot valid iff 0 <= idx < vis(b,t), empty slots anywhere that address no table entry and no pool row, a position listed twice two keys, no
 * valid slot O = 0 and LSE = -inf, T without a cap, Hq in 1 ... 128, any topk >= 1 -- on cln_fa2_decode_paged_mla_bf16_fp8's pool: codes
 * [P,page,576] of bytes and kv_scale fp32 [1] ON THE DEVICE, value = e4m3(code) kv_scale; the caller guarantees a finite kv_scale > 0 and no
 * NaN code in a LISTED row (an unlisted row is never read). The codes are converted to bf16 exactly on the way to LDS, once per workgroup; the
 * fp32 score multiplier is (softmax_scale log2 e) kv_scale and kv_scale multiplies the fp32 result in front of its store, so the partials of a
 * split carry it. With kv_scale a power of two O and LSE equal cln_fa2_decode_paged_mla_sparse_bf16's on the pool dequantised to bf16 bit for
 * bit; on the dense list [0 ... vis - 1, -1 ...] they equal cln_fa2_decode_paged_mla_bf16_fp8's.
 * Status, in the siblings' order: the scale (-1); a missing or misaligned pointer (q, pool, o, lse, workspace 16 bytes; block_table, seqlens,
 * kv_scale, indices 4 bytes) or an output equal to an input or another output (-1); P <= 0 (-1); the plan (-1 / -2 as there); a workspace
 * smaller than the plan's (-1). _plan returns what cln_fa2_decode_paged_mla_sparse_bf16_plan returns, status included. Deterministic.
 */
int cln_fa2_decode_paged_mla_sparse_bf16_fp8_plan(int B, int T, int Hq, int topk, int max_pages, int page, int* splits, int* chunk,
                                                  long long* workspace_bytes);
int cln_fa2_decode_paged_mla_sparse_bf16_fp8(const void* q, const void* pool, const int* block_table, const int* seqlens, const float* kv_scale,
                                             const int* indices, void* o, float* lse, void* workspace, long long workspace_bytes, int B, int T,
                                             int Hq, int topk, int P, int max_pages, int page, float softmax_scale, void* stream);
int cln_fa2_decode_paged_mla_sparse_bf16_fp8_describe(int B, int T, int Hq, int topk, int max_pages, int page, float softmax_scale, char* buf,
                                                      int len);

/* ---- The indexer's cache held in FP8 (OCP e4m3fn) with one fp32 scale per token: DeepSeek-V3.2's own format for
 * its index keys, 132 bytes a token where the bf16 pool stores 256. idx_pool is BYTES, [P, page, 132] to the caller, 16-byte aligned, behind the
 * block table and the lengths of the latent cache. Inside a page of 132 page bytes:
 *     bytes [0, 128 page)          codes  [page, 128] e4m3fn, token slot r at byte 128 r
 *     bytes [128 page, 132 page)   scales [page] fp32,        token slot r at byte 128 page + 4 r
 * (132 page is a multiple of 16 for every supported page, 16 ... 256: a code row is 16-byte aligned, a scale 4-byte aligned.) A stored token
 * means k_d = e4m3(code_d) scale. The layout as written here is the contract. cln_mla_index_topk and both sparse decodes take the results as
 * they are; nothing above changes.
 *
 * cln_kv_append_paged_index_bf16_fp8: cln_kv_append_paged_index_bf16 with a quantising store. Which row goes where is that entry's, word for
 * word (packed rows by cu_q clamped on the device, seqlens AFTER the append, liveness, a table entry outside [0, P) stores nothing, rows of no
 * sequence untouched); every byte of the pool that is not a live token's 128 codes or 4 scale bytes keeps its value. Per live token, all in
 * IEEE fp32: a = max(max_d |k_d|, 1e-4f); scale = a / 448.0f; if scale_pow2, scale = the smallest power of two >= scale (on the bits: mantissa
 * zero -> unchanged, else exponent + 1 and mantissa 0); inv = 1.0f / scale; code_d = e4m3fn, round to nearest even, of clamp(k_d inv, -448,
 * 448); the scale is stored as computed (always > 0). Inputs are finite: the caller's contract. scale_pow2 is 0 or 1; the model's
 * configuration uses 1 (ue8m0). Status, in this order: a missing or misaligned pointer (k_idx_new, idx_pool 16 bytes; the int arrays 4) or
 * idx_pool equal to an input (-1); P <= 0 (-1); scale_pow2 neither 0 nor 1 (-1); a non-positive B, total_q, max_pages or page (-1); another
 * page or max_pages page >= 2^31 (-2). _describe: buf / len (-1), scale_pow2 (-1), then the shape.
 *
 * cln_mla_index_logits_paged_bf16_fp8: cln_mla_index_logits_paged_bf16's argument list with this pool in place of the bf16 one; q_idx bf16
 * [B,T,Hi,128], weights fp32 [B,T,Hi], logits fp32 [B,T,ld]. With c_j the codes of position j read as numbers and s_j its scale it writes
 *     logits[b,t,j] = s_j sum_h weights[b,t,h] max(0, q_idx[b,t,h] . c_j)        for 0 <= j < vis(b,t)
 * and NOTHING ELSE; cap, vis and "no key, scale or table entry at or past vis is read" are the bf16 entry's rules. The scale is multiplied
 * once per key, after the head sum, in fp32: equal to the dequantise-then-ReLU form exactly for s_j >= 0. s_j finite and >= 0 and no NaN code
 * in a visible row are the caller's contract (what the append writes is > 0 and never NaN). The codes are converted to bf16 exactly on the
 * way into the matrix operand, so the products are exact in fp32; the order of operations depends on neither the grid, the batch nor the
 * length. Any T >= 1, Hi in 1 ... 64, no workspace. Status and order: cln_mla_index_logits_paged_bf16's.
 */
int cln_kv_append_paged_index_bf16_fp8(const void* k_idx_new, void* idx_pool, const int* block_table, const int* seqlens, const int* cu_q, int B,
                                       int total_q, int P, int max_pages, int page, int scale_pow2, void* stream);
int cln_kv_append_paged_index_bf16_fp8_describe(int B, int total_q, int max_pages, int page, int scale_pow2, char* buf, int len);
int cln_mla_index_logits_paged_bf16_fp8(const void* q_idx, const float* weights, const void* idx_pool, const int* block_table,
                                        const int* seqlens, float* logits, int B, int T, int Hi, long long ld, int P, int max_pages, int page,
                                        void* stream);
int cln_mla_index_logits_paged_bf16_fp8_describe(int B, int T, int Hi, long long ld, int max_pages, int page, char* buf, int len);

/* ---- The packed variable-length DSA step: the three calls behind the append -- indexer logits, exact top-k,
 * sparse MLA decode -- for the batch format the appends already take: [total_q, ...] rows and the offsets cu_q int32 [B + 1] ON THE DEVICE
 * (the cu_seqlens_q convention of cln_fa2_prefill_paged_varlen). One step of continuous batching, a prompt chunk next to single-token decode
 * rows, is then four calls whatever the mix, with no padding to a common T. Both caches, bf16 and FP8, are covered. Nothing above changes.
 *
 * One rule for all five entries. Packed row r < total_q belongs to sequence b, the largest b in [0, B) with cu_q[b] <= r; c0 = cu_q[b],
 * T_b = cu_q[b + 1] - c0, t = r - c0, and
 *     vis(r) = clamp(seqlens[b], 0, cap) - (T_b - 1 - t)
 * with each entry's own cap (min(max_pages page, ld); ld; max_pages page). seqlens holds the lengths AFTER the append. From there the
 * definition of the fixed-T entry holds word for word with row r in the place of (b, t): which logits are written, the dense list for
 * n <= topk, a slot valid iff 0 <= idx < vis, empty slots, every split written. T_b = 0 is legal: a sequence without a token this step. The
 * offsets are read through the clamp of cln_kv_append_paged_varlen -- every value to [0, total_q], T_b = max(., 0), the binary search over
 * the clamped values -- so a malformed cu_q (decreasing, negative, past total_q) is outside the contract and still addresses nothing but row
 * r < total_q. A row that belongs to no sequence (r < cu_q[0], r >= cu_q[B], or t >= T_b) reads no pool, table entry or length, and its
 * outputs are defined: logits nothing written; top-k all topk slots -1; sparse decode O = 0 and LSE = -inf, with splits every partial
 * written empty.
 *
 * Tensors: q_idx bf16 [total_q,Hi,128], weights fp32 [total_q,Hi], logits fp32 [total_q,ld], indices int32 [total_q,topk], q bf16
 * [total_q,Hq,576], o bf16 [total_q,Hq,512], lse fp32 [total_q,Hq] or NULL; pools, block_table [B,max_pages], seqlens [B], kv_scale, ld,
 * topk and softmax_scale as in the fixed-T entries. cu_q is 4-byte aligned and stands among the int inputs behind seqlens.
 *
 * With cu_q = [0, T, 2 T, ..., B T] every entry returns the bits of its fixed-T sibling on the same tensors, and the sparse _plan is the
 * sibling's: _plan(total_q, ...) equals cln_fa2_decode_paged_mla_sparse_bf16_plan(B, T, ...) for total_q = B T, status included. Grids:
 * total_q ceil(cap / 1024) workgroups (logits), total_q (top-k), total_q ceil(Hq / 64) S (sparse). Nothing is read on the host, nothing
 * is allocated: every entry can be captured into a graph, and cu_q and seqlens may change on the device between replays.
 *
 * Status, in the siblings' order with total_q in the place of B T. Logits: a missing or misaligned pointer (q_idx, idx_pool 16 bytes; weights,
 * block_table, seqlens, cu_q, logits 4) or logits equal to an input (-1); P <= 0 (-1); a non-positive B, total_q, Hi, ld, max_pages or page
 * (-1); Hi > 64, another page, max_pages page >= 2^31 or a grid that does not fit (-2). Top-k: a missing or misaligned pointer (all 4 bytes)
 * or indices equal to an input (-1); a non-positive B, total_q, ld or topk (-1); ld >= 2^31, topk total_q past 2^61 or a grid that does not
 * fit (-2). Sparse: the scale (-1); a missing or misaligned pointer (q, pool, o, lse, workspace 16 bytes; block_table, seqlens, cu_q,
 * [kv_scale,] indices 4) or an output equal to an input or another output (-1); P <= 0 (-1); a non-positive B, total_q, Hq or topk (-1);
 * Hq > 128, another page, max_pages page >= 2^31 or a grid that does not fit (-2); a workspace smaller than the plan's (-1). Deterministic.
 */
int cln_mla_index_logits_paged_varlen_bf16(const void* q_idx, const float* weights, const void* idx_pool, const int* block_table,
                                           const int* seqlens, const int* cu_q, float* logits, int B, int total_q, int Hi, long long ld, int P,
                                           int max_pages, int page, void* stream);
int cln_mla_index_logits_paged_varlen_bf16_describe(int B, int total_q, int Hi, long long ld, int max_pages, int page, char* buf, int len);
int cln_mla_index_logits_paged_varlen_bf16_fp8(const void* q_idx, const float* weights, const void* idx_pool, const int* block_table,
                                               const int* seqlens, const int* cu_q, float* logits, int B, int total_q, int Hi, long long ld,
                                               int P, int max_pages, int page, void* stream);
int cln_mla_index_logits_paged_varlen_bf16_fp8_describe(int B, int total_q, int Hi, long long ld, int max_pages, int page, char* buf, int len);
int cln_mla_index_topk_varlen(const float* logits, const int* seqlens, const int* cu_q, int* indices, int B, int total_q, long long ld, int topk,
                              void* stream);
int cln_mla_index_topk_varlen_describe(int B, int total_q, long long ld, int topk, char* buf, int len);
int cln_fa2_decode_paged_mla_sparse_varlen_bf16_plan(int total_q, int Hq, int topk, int max_pages, int page, int* splits, int* chunk,
                                                     long long* workspace_bytes);
int cln_fa2_decode_paged_mla_sparse_varlen_bf16(const void* q, const void* pool, const int* block_table, const int* seqlens, const int* cu_q,
                                                const int* indices, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                                                int total_q, int Hq, int topk, int P, int max_pages, int page, float softmax_scale,
                                                void* stream);
int cln_fa2_decode_paged_mla_sparse_varlen_bf16_describe(int B, int total_q, int Hq, int topk, int max_pages, int page, float softmax_scale,
                                                         char* buf, int len);
int cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan(int total_q, int Hq, int topk, int max_pages, int page, int* splits, int* chunk,
                                                         long long* workspace_bytes);
int cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8(const void* q, const void* pool, const int* block_table, const int* seqlens,
                                                    const int* cu_q, const float* kv_scale, const int* indices, void* o, float* lse,
                                                    void* workspace, long long workspace_bytes, int B, int total_q, int Hq, int topk, int P,
                                                    int max_pages, int page, float softmax_scale, void* stream);
int cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_describe(int B, int total_q, int Hq, int topk, int max_pages, int page,
                                                             float softmax_scale, char* buf, int len);

#ifdef __cplusplus
}
#endif
#endif /* CLN_AMD_EXT_H */
