// MXFP4-weight GEMM on the scaled FP4 x FP8 matrix instruction of gfx950 (cln_gemm_mxfp4_bf16, include/cln_amd_ext.h):
//   out[m, n] = bf16_rne( bias[n] + sum_{kb < K/32} 2^(sa[m, kb] - 127) 2^(sb[n, kb] - 127) sum_{k in block kb} e4m3(a[m, k]) e2m1(b[n, k]) )
// a [M, K] e4m3fn with a_scale e8m0 [M, K/32] (what cln_quant_mxfp8_bf16 writes), b [N, K/2] two e2m1 codes a byte with b_scale e8m0 [N, K/32]
// (a gpt-oss expert's `_blocks` / `_scales` as stored), bias bf16 [N] or none, out bf16 [M, N]. One rounding to bf16 at the store, one 8-byte
// bf16 x 4 per lane and sub-tile, aligned because N % 8 == 0.
//
// This header owns the dense kernel template, its plan and its launch. The instruction, the orientation, both bodies (gx4::skinny<MT>,
// gx4::tile) and their register and bank arithmetic are gemm_mxfp4_core.cuh's, which the grouped form includes without this file.
//
// ONE kernel template, gemm_mxfp4_mfma<TILE, MT>, two forms; form 0 picks by M alone (M <= 64: skinny), 1 and 2 pin one.
// SKINNY (TILE = false): strips of 32 or 64 weight rows (32 when 64-row strips would leave CUs without a workgroup) x all of M in chunks of
// 16 MT rows (one chunk for M <= 64; a pinned skinny form on more rows re-reads its strip per chunk, from L2). TILE (TILE = true): output
// tiles of 128 x 128 from row 128 blockIdx.y, 51200 bytes of static LDS.
#pragma once
#include "gemm_mxfp4_core.cuh"
#include "gemm_fp8_block128_offsets.cuh"  // g8o::kAuto, kSkinny, kTile: the family's form codes

namespace gx4 {

template <bool TILE, int MT>
__global__ __launch_bounds__(256) void gemm_mxfp4_mfma(const Args a) {
  if constexpr (TILE) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[kTileLds];
    tile(a, kTileM * blockIdx.y, smem);
  } else {
    skinny_rows<MT>(a);
  }
}

// ---- the plan: a function of the shape and the form only (the entry and its describe share it)
struct Plan {
  int tile;   // 1: the tile form
  int mt;     // skinny: 16-row activation sub-tiles a chunk
  int waves;  // waves a workgroup (skinny: 2 or 4 = a strip of 32 or 64 weight rows)
  unsigned gx, gy;
};

inline bool shape_ok(long long M, long long N, long long K) {
  return M >= 1 && N >= 8 && N % 8 == 0 && K >= kMx && K % kMx == 0 && M <= 0x7fffffffLL && N <= 0x7fffffffLL - 256 && K <= 0x3fffffffLL;  // 128 (K / 128 + kPF + 1) stays an int
}

// -2 for a shape outside the contract or past one launch in the form chosen; then -1 for a form that is none of 0, 1, 2
inline int plan(long long M, long long N, long long K, int form, Plan* p) {
  if (!shape_ok(M, N, K)) return CLN_ERR_UNSUPPORTED;
  p->tile = !(form == g8o::kSkinny || (form != g8o::kTile && M <= kSkinnyMaxM));
  if (!p->tile) {
    p->mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
    p->waves = (N + 63) / 64 >= kCUs ? 4 : 2;  // 64-row strips only where they still give every CU a workgroup
    p->gx = (unsigned)((N + 16 * p->waves - 1) / (16 * p->waves));
    p->gy = 1;
  } else {
    p->mt = 4;
    p->waves = 4;
    p->gx = (unsigned)((N + kTileN - 1) / kTileN);
    const long long gy = (M + kTileM - 1) / kTileM;
    if (gy > g8o::kMaxGridY) return CLN_ERR_UNSUPPORTED;
    p->gy = (unsigned)gy;
  }
  return form == g8o::kAuto || form == g8o::kSkinny || form == g8o::kTile ? CLN_OK : CLN_ERR_BAD_ARG;
}

inline int launch(const Args& a, const Plan& p, hipStream_t stream) {
  const dim3 grid(p.gx, p.gy), block(64 * p.waves);
  if (p.tile) CLN_LAUNCH((gemm_mxfp4_mfma<true, 4>), grid, block, 0, stream, a);
  else if (p.mt == 1) CLN_LAUNCH((gemm_mxfp4_mfma<false, 1>), grid, block, 0, stream, a);
  else if (p.mt == 2) CLN_LAUNCH((gemm_mxfp4_mfma<false, 2>), grid, block, 0, stream, a);
  else CLN_LAUNCH((gemm_mxfp4_mfma<false, 4>), grid, block, 0, stream, a);
  return cln_check_launch();
}

}  // namespace gx4
