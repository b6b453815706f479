// Packed variable-length prefill attention with bf16 queries over a PAGED KV cache held in FP8 (OCP e4m3fn, one fp32 scale per KV head) with a
// SLIDING WINDOW and optional ATTENTION SINKS (cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8, include/cln_amd_ext.h):
// the shared statements (flash_attn_prefill_paged_varlen_window_body.cuh, which has the staging stage of the FP8 pools and says where k_scale
// and v_scale enter) on fa2d::PagedKV8, with G = 2^g_shift. sinks may be null: no sink, the bits of sinks that are all -inf.
#pragma once
#include "flash_attn_prefill_paged_varlen_window_body.cuh"

namespace fa2b {

template <int D>
__global__ __launch_bounds__(kThreads, 2) void fa2_prefill_paged_varlen_window_sink_bf16_fp8_mfma(
    const bf16_t* __restrict__ q, const fa2d::PagedKV8 kv, const int* __restrict__ seqlens, const int* __restrict__ cu_q,
    const float* __restrict__ sinks, bf16_t* __restrict__ o, float* __restrict__ lse, int B, int total_q, int g_shift, unsigned slots, int W,
    float scale_log2) {
  static_assert(D == 64 || D == 128, "head dim");
  using GM = GroupPow2;
  constexpr Sinks SINKS = Sinks::kOptional;
  constexpr bool CAP = false;
  constexpr float pre = 0.0f, cap2 = 0.0f;  // CAP only
  const int ga = g_shift;
#include "flash_attn_prefill_paged_varlen_window_body.inc"
}

// launch_prefill_paged_varlen_window_sink over the e4m3 pools; sinks may be null
template <int D>
int launch_prefill_paged_varlen_window_sink_fp8(const void* q, const fa2d::PagedKV8& kv, const int* seqlens, const int* cu_q, const float* sinks,
                                                void* o, float* lse, int B, int total_q, int g_shift, long long slots, int W, hipStream_t stream) {
  CLN_LAUNCH((fa2_prefill_paged_varlen_window_sink_bf16_fp8_mfma<D>), dim3((unsigned)((long long)kv.Hkv * slots)), dim3(kThreads), 0, stream,
             (const bf16_t*)q, kv, seqlens, cu_q, sinks, (bf16_t*)o, lse, B, total_q, g_shift, (unsigned)slots, W, fa2d::scale_log2(D));
  return cln_check_launch();
}

}  // namespace fa2b
