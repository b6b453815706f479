// The scale of one block of values that is quantised to FP8 (OCP e4m3fn) from its largest magnitude, all in IEEE fp32:
//   a     = max(amax, 1e-4f)
//   scale = a / 448.0f
//   if pow2: scale = the smallest power of two >= scale -- on the bits: mantissa zero -> unchanged, else exponent + 1, mantissa 0 (no log2)
// scale >= 1e-4 / 448 > 0 always. The one statement of the rule: the activation quantiser (quant_fp8_block128_bf16.cuh), the fused gate/up
// epilogue (gemm_fp8_block128_grouped_swiglu.cuh), the per-token index-key append (kv_append_paged_index_bf16_fp8.cuh) and the per-tile latent
// append (kv_append_paged_mla_bf16_fp8_tile.cuh) call it, so a block of the same values gets the same scale bits from all four. Defines no kernel.
#pragma once
#include "common.h"

__device__ __forceinline__ float cln_fp8_block_scale(float amax, int pow2) {
  float scale = fmaxf(amax, 1e-4f) / 448.0f;
  if (pow2) {
    const unsigned bits = __float_as_uint(scale);  // positive and normal
    if (bits & 0x007fffffu) scale = __uint_as_float((bits & 0x7f800000u) + 0x00800000u);
  }
  return scale;
}
