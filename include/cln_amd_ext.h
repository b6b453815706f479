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

#ifdef __cplusplus
}
#endif
#endif /* CLN_AMD_EXT_H */
