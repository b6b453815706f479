// What the two MFMA attention kernels over an FP8 (OCP e4m3fn) paged KV cache share (flash_attn_prefill_paged_fp8.cuh,
// flash_attn_decode_paged_multi_fp8.cuh): the conversion of stored bytes to halves. Every e4m3 value (4 exponent bits, 3 mantissa bits,
// subnormals down to 2^-9) is an fp16 value, so the halves hold the UNSCALED codes exactly and the fp16 MFMA body runs on them unchanged; the
// per-head scales stay outside the loop (k_scale in the score multiplier, v_scale in the normalisation). The pool view is fa2d::PagedKV8.
#pragma once
#include "flash_attn_decode_paged_fp8.cuh"

namespace fa2d {

// 8 e4m3fn bytes -> 8 halves, in memory order: one v_cvt_scalef32_pk_f16_fp8 (scale 2^0) per two elements
__device__ __forceinline__ h8 e4m3x8_to_h8(uint2 b) {
  const h2 a0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)b.x, 1.0f, false), a1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)b.x, 1.0f, true);
  const h2 a2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)b.y, 1.0f, false), a3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)b.y, 1.0f, true);
  return h8{a0[0], a0[1], a1[0], a1[1], a2[0], a2[1], a3[0], a3[1]};
}

}  // namespace fa2d
