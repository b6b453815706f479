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

#ifdef __cplusplus
}
#endif
#endif /* CLN_AMD_EXT_H */
