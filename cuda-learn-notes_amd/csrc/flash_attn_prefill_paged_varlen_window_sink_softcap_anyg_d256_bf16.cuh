// Packed variable-length prefill attention over a PAGED KV cache in bf16 at HEAD DIM 256, with a sliding window, optional attention sinks, any
// query-group size G = Hq / Hkv in 1 ... 16, a softmax scale of the caller's and optional logit soft-capping
// (cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16, include/cln_amd_ext.h): the statements of
// fa2b::fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_mfma (flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_bf16.cuh), which
// takes D = 64 and 128, under launch bounds of its own. The semantics, the masks, the order cap -> mask, the sink and the epilogue are that
// kernel's.
//
// The budget that decides the layout (registers per lane, 32-bit; DESIGN 4.4.16 has the table with the compiler's numbers):
//   per 16-row tile   64 accumulators (16 f4), 32 of Q fragments (8 b8), 16 of scores (4 f4), 8 of P (2 b8)
//   per thread        a 64-key step staged through registers: 8 pieces of 16 bytes per tensor = 32 for K and 32 for V, live from the load in
//                     one step to the LDS store in the next; 32 of K fragments (8 b8) per 16-key block while the scores are formed
// The workgroup tile stays 128 rows -- four waves of two 16-row tiles, kMT = 2 -- so seq_of_slot_anyg, slot_of_anyg and slots = total_q G / 128 + B
// serve unchanged and a staged K / V step feeds 128 rows as at D = 128: 2 (64 + 32 + 16 + 8) + 64 + 32 = 336 registers before addresses and the
// softmax temporaries. That is past the 256 architectural VGPRs, so the kernel asks for one wave per SIMD (__launch_bounds__(256, 1)), which on
// gfx950 gives a wave the unified file of 512: the MFMA accumulators take AGPRs as their C / D operand directly, and nothing is spilled. The
// alternative, a 64-row tile at two waves per SIMD, halves the rows a staged step feeds (every K fragment read from LDS then feeds one MFMA
// instead of two) and needs slot helpers of its own; it was not taken. MEASURED: this layout runs at 2.1 - 5.7 times the
// D = 128 kernel's time where 2.0 was the reference point -- one wave per SIMD costs more than the shared tile saves. A layout at two waves per
// SIMD (eight waves of one 16-row tile on this same tile and LDS image, or the 64-row tile) is the next step.
// LDS: K and V of a 64-key step in rows of 2 D + 32 = 544 bytes (the padding that keeps the transposing reads off each other's banks):
// 2 x 64 x 544 = 69632 bytes, static. One workgroup per CU.
// Per step and wave: 4 key blocks x 2 row tiles x 8 k-steps = 64 MFMAs for S^T and 2 x 16 dim blocks x 2 row tiles = 64 for O^T, all
// v_mfma_f32_16x16x32_bf16.
// The statements are the shared ones (flash_attn_prefill_paged_varlen_window_body.inc); at 505 / 512 VGPRs this kernel has no slack, and it
// goes through them because the inclusion leaves its instruction stream as it was, byte for byte.
#pragma once
#include "flash_attn_prefill_paged_varlen_window_body.cuh"

namespace fa2b {

constexpr int kHeadDim256 = 256;
constexpr int kPrefill256LdsBytes = 2 * kKeyStep * (2 * kHeadDim256 + 32);

template <bool CAP>
__global__ __launch_bounds__(kThreads, 1) void fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_mfma(
    const bf16_t* __restrict__ q, const PagedKV kv, const int* __restrict__ seqlens, const int* __restrict__ cu_q, const float* __restrict__ sinks,
    bf16_t* __restrict__ o, float* __restrict__ lse, int B, int total_q, int G, unsigned slots, int W, float scale_log2, float pre, float cap2) {
  constexpr int D = kHeadDim256;
  static_assert(2 * kKeyStep * (2 * D + 32) == kPrefill256LdsBytes, "the describe text states this");
  using GM = GroupAny;
  constexpr Sinks SINKS = Sinks::kOptional;
  const int ga = G;
#include "flash_attn_prefill_paged_varlen_window_body.inc"
}

template <bool CAP>
int launch_prefill_paged_varlen_window_sink_softcap_anyg_d256(const void* q, const PagedKV& kv, const int* seqlens, const int* cu_q,
                                                              const float* sinks, void* o, float* lse, int B, int total_q, int G, long long slots,
                                                              int W, float mult, float pre, float cap2, hipStream_t stream) {
  CLN_LAUNCH((fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_mfma<CAP>), dim3((unsigned)((long long)kv.Hkv * slots)), dim3(kThreads), 0,
             stream, (const bf16_t*)q, kv, seqlens, cu_q, sinks, (bf16_t*)o, lse, B, total_q, G, (unsigned)slots, W, mult, pre, cap2);
  return cln_check_launch();
}

}  // namespace fa2b
