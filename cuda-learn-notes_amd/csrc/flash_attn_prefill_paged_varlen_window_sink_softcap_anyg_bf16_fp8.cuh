// Packed variable-length prefill attention with bf16 queries over a PAGED KV cache held in FP8 (OCP e4m3fn, one fp32 scale per KV head) with a
// SLIDING WINDOW, optional ATTENTION SINKS, any query-group size G = Hq / Hkv in 1 ... 16, a SOFTMAX SCALE of the caller's and optional LOGIT
// SOFT-CAPPING (cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8, include/cln_amd_ext.h):
// the shared statements (flash_attn_prefill_paged_varlen_window_body.cuh, which says why k_scale stands inside the tanh) on fa2d::PagedKV8
// with the caller's multipliers and the compile-time flag CAP.
#pragma once
#include "flash_attn_prefill_paged_varlen_window_body.cuh"

namespace fa2b {

template <int D, bool CAP>
__global__ __launch_bounds__(kThreads, 2) void fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8_mfma(
    const bf16_t* __restrict__ q, const fa2d::PagedKV8 kv, const int* __restrict__ seqlens, const int* __restrict__ cu_q,
    const float* __restrict__ sinks, bf16_t* __restrict__ o, float* __restrict__ lse, int B, int total_q, int G, unsigned slots, int W,
    float scale_log2, float pre, float cap2) {
  static_assert(D == 64 || D == 128, "head dim");
  using GM = GroupAny;
  constexpr Sinks SINKS = Sinks::kOptional;
  const int ga = G;
#include "flash_attn_prefill_paged_varlen_window_body.inc"
}

// launch_prefill_paged_varlen_window_sink_anyg_fp8 with the multipliers of paged::softcap_arg; CAP = false without a cap
template <int D, bool CAP>
int launch_prefill_paged_varlen_window_sink_softcap_anyg_fp8(const void* q, const fa2d::PagedKV8& kv, const int* seqlens, const int* cu_q,
                                                             const float* sinks, void* o, float* lse, int B, int total_q, int G, long long slots,
                                                             int W, float mult, float pre, float cap2, hipStream_t stream) {
  CLN_LAUNCH((fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8_mfma<D, CAP>), dim3((unsigned)((long long)kv.Hkv * slots)), dim3(kThreads),
             0, stream, (const bf16_t*)q, kv, seqlens, cu_q, sinks, (bf16_t*)o, lse, B, total_q, G, (unsigned)slots, W, mult, pre, cap2);
  return cln_check_launch();
}

}  // namespace fa2b
