// Block-scaled FP8 (OCP e4m3fn) GEMM on the FP8 matrix pipe of gfx950 (cln_gemm_fp8_block128_bf16, include/cln_amd_ext.h):
//   out[m, n] = bf16_rne( sum_kb  a_scale[m, kb] * b_scale[n / 128, kb] * sum_{k in block kb} fp32(a[m, k]) * fp32(b[n, k]) )
// a [M, K] e4m3fn with a_scale fp32 [M, K/128] (per token and 128 columns), b [N, K] e4m3fn (the nn.Linear weight as stored) with b_scale fp32
// [ceil(N/128), K/128] (128 x 128 blocks), out bf16 [M, N]: DeepSeek-V3's projection format. One rounding to bf16 at the store, one 8-byte
// bf16 x 4 per lane and sub-tile, aligned because N % 8 == 0.
//
// This header owns the dense kernel template, its plan and its launch. The arithmetic, the orientation, both bodies (g8::skinny<MT>,
// g8::tile) and their register and bank arithmetic are gemm_fp8_block128_core.cuh's, which the grouped forms include without this file.
//
// ONE kernel template, gemm_fp8_block128_mfma<TILE, MT>, two forms; the host picks by M alone (M <= 64: skinny).
// SKINNY (TILE = false; decode: N K bytes once against 2 M N K flops): strips of 32 or 64 weight rows (32 when 64-row strips would leave CUs
// without a workgroup) x all of M padded to 16 MT rows. TILE (TILE = true; prefill): output tiles of 128 x 128 from row 128 blockIdx.y,
// 66560 bytes of static LDS.
#pragma once
#include "gemm_fp8_block128_core.cuh"

namespace g8 {

template <bool TILE, int MT>
__global__ __launch_bounds__(256) void gemm_fp8_block128_mfma(const Args a) {
  if constexpr (TILE) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[kTileLds];
    tile(a, kTileM * blockIdx.y, smem);
  } else {
    skinny<MT>(a);
  }
}

// ---- the plan: a function of the shape only (the entry and its describe share it)
struct Plan {
  int tile;     // 1: the tile form
  int mt;       // skinny: 16-row activation sub-tiles (M padded to 16 mt)
  int waves;    // waves a workgroup (skinny: 2 or 4 = a strip of 32 or 64 weight rows)
  unsigned gx, gy;
};

inline int plan(long long M, long long N, long long K, Plan* p) {
  if (M < 1 || N < 8 || N % 8 || K < kBlock || K % kBlock) return CLN_ERR_UNSUPPORTED;
  if (M > 0x7fffffffLL || N > 0x7fffffffLL - 256 || K > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  if (M <= kSkinnyMaxM) {
    p->tile = 0;
    p->mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
    p->waves = (N + 63) / 64 >= kCUs ? 4 : 2;  // 64-row strips only where they still give every CU a workgroup
    p->gx = (unsigned)((N + 16 * p->waves - 1) / (16 * p->waves));
    p->gy = 1;
  } else {
    p->tile = 1;
    p->mt = 4;
    p->waves = 4;
    p->gx = (unsigned)((N + kTileN - 1) / kTileN);
    const long long gy = (M + kTileM - 1) / kTileM;
    if (gy > 65535) return CLN_ERR_UNSUPPORTED;
    p->gy = (unsigned)gy;
  }
  return CLN_OK;
}

inline int launch(const Args& a, const Plan& p, hipStream_t stream) {
  const dim3 grid(p.gx, p.gy), block(64 * p.waves);
  if (p.tile) CLN_LAUNCH((gemm_fp8_block128_mfma<true, 4>), grid, block, 0, stream, a);
  else if (p.mt == 1) CLN_LAUNCH((gemm_fp8_block128_mfma<false, 1>), grid, block, 0, stream, a);
  else if (p.mt == 2) CLN_LAUNCH((gemm_fp8_block128_mfma<false, 2>), grid, block, 0, stream, a);
  else CLN_LAUNCH((gemm_fp8_block128_mfma<false, 4>), grid, block, 0, stream, a);
  return cln_check_launch();
}

}  // namespace g8
