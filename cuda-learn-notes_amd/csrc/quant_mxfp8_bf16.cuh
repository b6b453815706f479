// The activation quantiser of the MXFP4-weight GEMMs (cln_quant_mxfp8_bf16, include/cln_amd_ext.h): x bf16 [M, K] -> codes
// e4m3fn [M, K] and scale bytes e8m0 [M, K/32], one scale per row and 32 columns: the A operand of cln_gemm_mxfp4[_grouped]_bf16 (OCP MXFP8).
//
// Per row and 32-column block, in integer and IEEE fp32 operations (the OCP MX "floor" rule with emax(e4m3) = 8):
//   E     = the biased exponent field (bits 30 ... 23) of fp32(max |x|)
//   scale = clamp(E - 8, 0, 254)                                                   (the e8m0 byte: 2^(scale - 127))
//   inv   = 2^(127 - scale), built on its bits                                     (exact; scale = 254 gives the subnormal 2^-127)
//   code  = e4m3fn, round to nearest even, of clamp(x inv, -448, 448)              (kva::store_fp8, as it stands)
// so amax = 0 (and any amax below 2^-118, a subnormal one included) gives scale byte 0, and a scaled magnitude in (448, 512) saturates to
// 448, as the MX specification says. Inputs are finite: the caller's contract.
//
// 4 threads a block: a thread loads 16 bytes (8 columns), the block's amax goes over its 4 lanes by two DPP moves inside the quad.
// u = 4 blk + j with j = lane & 3, and the one early return tests blk only: the 4 lanes of a quad leave or stay together. Lane 0 of the quad
// stores the scale byte. Block blk = row K/32 + kb sits at element 32 blk of x and codes and at scales[blk]: the three tensors are
// contiguous. Bandwidth-bound; no LDS, no atomics, one launch.
#pragma once
#include "kv_append_paged_fp8.cuh"  // kva::store_fp8, kva::kThreads
#include "paged_bf16.cuh"

namespace qmx {

struct Args {
  const bf16_t* x;
  uint8_t *codes, *scales;
  long long blocks;  // M * K / 32
};

// One thread's share of one MX block, the per-block rule above: 8 columns at x8 / codes8 (the block's start + 8 j, j the lane's place in the
// block's quad, whose 4 lanes call together); lane 0 of the quad stores the scale byte. The row kernel (quant_mxfp8_bf16.hip) and the
// gathering form (moe_dispatch.cuh) both call it, so a row carries the same bits from both. This header defines no kernel.
__device__ __forceinline__ void quant_piece(const bf16_t* x8, uint8_t* codes8, uint8_t* scale_out, unsigned j) {
  const b8 x = *(const b8*)x8;
  float y[8];
  float m = 0.0f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    y[e] = (float)x[e];
    m = fmaxf(m, fabsf(y[e]));
  }
  m = fmaxf(m, cln_dpp<0xB1>(m));  // quad_perm [1,0,3,2]
  m = fmaxf(m, cln_dpp<0x4E>(m));  // quad_perm [2,3,0,1]: the block's amax in its 4 lanes
  const int scale = min(max((int)((__float_as_uint(m) >> 23) & 0xFFu) - 8, 0), 254);
  const float inv = __uint_as_float(scale < 254 ? (unsigned)(254 - scale) << 23 : 0x00400000u);
  kva::store_fp8(codes8, y, inv);
  if (j == 0) *scale_out = (uint8_t)scale;
}

// workgroups of the launch, or 0 when the shape does not fit one launch
inline long long workgroups(long long blocks) {
  const long long wgs = (blocks * 4 + kva::kThreads - 1) / kva::kThreads;
  return wgs <= 0x7fffffffLL ? wgs : 0;
}

}  // namespace qmx
