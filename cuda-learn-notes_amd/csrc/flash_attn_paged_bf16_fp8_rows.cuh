// What the two MFMA attention kernels over an FP8 (OCP e4m3fn) paged KV cache with bf16 queries share
// (flash_attn_prefill_paged_varlen_window_sink_bf16_fp8.cuh, flash_attn_decode_paged_multi_window_sink_bf16_fp8.cuh): the conversion
// of stored bytes to bf16, the twin of fa2d::e4m3x8_to_h8 (flash_attn_paged_fp8_rows.cuh), and the sink of a head where sinks may be null.
// Every e4m3 value (3 mantissa bits, exponents 2^-9 .. 2^8) is a bf16 value (7 mantissa bits, 8 exponent bits), so the bf16 elements hold the
// UNSCALED codes exactly and the bf16 MFMA body runs on them unchanged; the per-head scales stay outside the loop (k_scale in the score
// multiplier, v_scale in the normalisation). The pool view is fa2d::PagedKV8. Nothing passes through fp16.
#pragma once
#include "flash_attn_decode_paged_multi_window_sink_bf16.cuh"  // sink_log2, fold_sink; paged_bf16.cuh
#include "flash_attn_paged_fp8_rows.cuh"

namespace fa2b {

typedef __bf16 b2 __attribute__((ext_vector_type(2)));

// 8 e4m3fn bytes -> 8 bf16, in memory order: one v_cvt_scalef32_pk_bf16_fp8 (scale 2^0) per two elements
__device__ __forceinline__ b8 e4m3x8_to_b8(uint2 b) {
  const b2 a0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)b.x, 1.0f, false), a1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)b.x, 1.0f, true);
  const b2 a2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)b.y, 1.0f, false), a3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)b.y, 1.0f, true);
  return b8{a0[0], a0[1], a1[0], a1[1], a2[0], a2[1], a3[0], a3[1]};
}

// The sink of a head in the units of m, or -inf where the caller gave no sinks (-inf * log2 e = -inf: the bits of a sinks tensor of -inf)
__device__ __forceinline__ float sink_log2_or_none(const float* __restrict__ sinks, unsigned head) {
  return sinks ? sink_log2(sinks, head) : FA2D_NEG_INF;
}

}  // namespace fa2b
