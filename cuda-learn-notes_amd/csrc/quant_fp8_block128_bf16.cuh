// The activation quantiser of the block-scaled FP8 GEMM (cln_quant_fp8_block128_bf16, include/cln_amd_ext.h): x bf16 [M, K] ->
// codes e4m3fn [M, K] and scales fp32 [M, K/128], one scale per row and 128 columns: the A operand of cln_gemm_fp8_block128_bf16.
//
// Per row and 128-column block, all in IEEE fp32:
//   scale = cln_fp8_block_scale(max |x|, pow2)                                      (fp8_block_scale.cuh: max(amax, 1e-4) / 448, pow2 on the bits)
//   inv   = 1.0f / scale
//   code  = e4m3fn, round to nearest even, of clamp(x inv, -448, 448)              (kva::store_fp8, as it stands)
// and the scale is stored as computed. Inputs are finite: the caller's contract.
//
// 16 threads a block: a thread loads 16 bytes (8 columns), the block's amax goes over its 16 lanes by four DPP moves inside the 16-lane row.
// u = 16 blk + j with j = lane & 15, and the one early return tests blk only: the 16 lanes of a DPP row leave or stay together. Lane 0 of the
// row stores the scale. Block blk = row KB + kb sits at element 128 blk of x and codes and at scales[blk]: the three tensors are contiguous.
// Bandwidth-bound; no LDS, no atomics, one launch.
#pragma once
#include "fp8_block_scale.cuh"
#include "kv_append_paged_fp8.cuh"  // kva::store_fp8, kva::kThreads
#include "paged_bf16.cuh"

namespace q8 {

struct Args {
  const bf16_t* x;
  uint8_t* codes;
  float* scales;
  long long blocks;  // M * K / 128
  int pow2;
};

// One thread's share of one block, the per-block rule above: 8 columns at x8 / codes8 (the block's start + 8 j, j the lane's place among the
// block's 16 lanes, which call together); lane 0 of the block stores the scale. The row kernel (quant_fp8_block128_bf16.hip) and the gathering
// form (moe_dispatch.cuh) both call it, so a row carries the same bits from both. This header defines no kernel.
__device__ __forceinline__ void quant_piece(const bf16_t* x8, uint8_t* codes8, float* scale_out, unsigned j, int pow2) {
  const b8 x = *(const b8*)x8;
  float y[8];
  float m = 0.0f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    y[e] = (float)x[e];
    m = fmaxf(m, fabsf(y[e]));
  }
  m = fmaxf(m, cln_dpp<0xB1>(m));   // quad_perm [1,0,3,2]
  m = fmaxf(m, cln_dpp<0x4E>(m));   // quad_perm [2,3,0,1]
  m = fmaxf(m, cln_dpp<0x141>(m));  // row_half_mirror
  m = fmaxf(m, cln_dpp<0x140>(m));  // row_mirror: the block's amax in its 16 lanes
  const float scale = cln_fp8_block_scale(m, pow2);
  const float inv = 1.0f / scale;
  kva::store_fp8(codes8, y, inv);
  if (j == 0) *scale_out = scale;
}

// workgroups of the launch, or 0 when the shape does not fit one launch
inline long long workgroups(long long blocks) {
  const long long wgs = (blocks * 16 + kva::kThreads - 1) / kva::kThreads;
  return wgs <= 0x7fffffffLL ? wgs : 0;
}

}  // namespace q8
