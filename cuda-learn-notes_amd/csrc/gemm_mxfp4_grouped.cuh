// Grouped (mixture-of-experts) MXFP4-weight GEMM over expert offsets that live on the device (cln_gemm_mxfp4_grouped_bf16,
// include/cln_amd_ext.h): the rows of a [M_total, K] are sorted by expert, expert e owns the rows off[e] ... off[e + 1] - 1, its
// own weight b[e] [N, K/2], scale bytes b_scale[e] [N, K/32] and bias[e] [N]: the expert tensors of gpt-oss as stored. For a row m of expert e
//   out[m, n] = bf16_rne( bias[e, n] + sum_kb 2^(sa[m, kb] - 127) 2^(sb[e, n, kb] - 127) sum_{k in block kb} e4m3(a[m, k]) e2m1(b[e, n, k]) )
// This header owns the two grouped kernels, the view of one expert, the plan and the launch. Both bodies are the dense form's
// (gemm_mxfp4_core.cuh: gx4::skinny<MT>, gx4::tile) called on a view of the expert, so an expert's rows carry the bits the dense entry gives on
// that expert alone, in either form. How the work is found and split when the host cannot see the offsets -- the clamp, the slots, the
// search, the form rule -- is gemm_fp8_block128_offsets.cuh's (g8o), by inclusion: the contract is gemm_fp8_block128_grouped_bf16's.
//
// SKINNY. Grid (strips of 32 or 64 weight rows) x E: workgroup (x, e) owns strip x of expert e's weight and ALL of the expert's rows, and
// returns before its first weight load when M_e = 0. Otherwise it walks the expert's rows in chunks of up to 64; per chunk MT in {1, 2, 4}
// comes from the rows left (a workgroup-uniform branch over gx4::skinny's three instantiations). No LDS, no barrier.
// TILE. Tiles of 128 x 128, N tiles in x, the slots of g8o in y; gx4::tile on a view of the expert (M = M_e) with the tile's first row 128 t
// relative to the expert: rows clamped on load to the expert's OWN last row, stores masked at the expert's end.
// Element offsets are 64-bit, e N K / 2 included. One launch, nothing read on the host, no workspace, no atomics; deterministic;
// graph-capturable with the offsets changing between replays.
#pragma once
#include "gemm_mxfp4_core.cuh"
#include "gemm_fp8_block128_offsets.cuh"

namespace gx4g {

using gx4::kMx;
using gx4::kTileM;
using gx4::kTileN;

struct Args {
  const uint8_t *a, *b;    // [M,K] e4m3fn, [E,N,K/2] two e2m1 a byte
  const uint8_t *sa, *sb;  // [M,K/32], [E,N,K/32] e8m0
  const bf16_t* bias;      // [E,N], or null
  const int* off;          // [E + 1], on the device
  bf16_t* out;             // [M,N]
  int M, E, N, K;          // M = M_total
};

// The dense kernel's arguments on expert e alone: its weight, scales and bias, and its rows from row c0 + m0 on, `rows` of them.
__device__ __forceinline__ gx4::Args expert_view(const Args& g, int e, int c0, int m0, int rows) {
  const size_t r0 = (size_t)c0 + (size_t)m0, en = (size_t)e * (size_t)g.N;
  return {g.a + r0 * (size_t)g.K, g.b + en * (size_t)(g.K / 2), g.sa + r0 * (size_t)(g.K / kMx), g.sb + en * (size_t)(g.K / kMx),
          g.bias ? g.bias + en : nullptr, g.out + r0 * (size_t)g.N, rows, g.N, g.K};
}

// ---- the skinny form: grid (strips, E), blockDim.x = 64 W
__global__ __launch_bounds__(256) void gemm_mxfp4_grouped_skinny_mfma(const Args g) {
  const int e = blockIdx.y;
  const g8o::Rows r = g8o::expert_rows(g.off, g.M, e);
  if (r.Me == 0) return;  // the empty-expert exit: nothing of b[e] has been addressed
  for (int m0 = 0; m0 < r.Me; m0 += 64) {
    const int rows = min(64, r.Me - m0);
    const gx4::Args d = expert_view(g, e, r.c0, m0, rows);
    if (rows <= 16) gx4::skinny<1>(d);
    else if (rows <= 32) gx4::skinny<2>(d);
    else gx4::skinny<4>(d);
  }
}

// ---- the tile form: grid (N tiles, slots)
__global__ __launch_bounds__(256) void gemm_mxfp4_grouped_tile_mfma(const Args g) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[gx4::kTileLds];
  g8o::Tile w;
  if (!g8o::tile_of_slot(g.off, g.M, g.E, blockIdx.y, &w)) return;  // uniform, before any barrier
  gx4::tile(expert_view(g, w.e, w.c0, 0, w.Me), kTileM * w.t, smem);  // masked at the view's M = the expert's end
}

// ---- the plan: a function of (M_total, E, N, K, form) only (the entry and its describe share it)
struct Plan {
  int tile;   // 1: the tile form
  int waves;  // waves a workgroup (skinny: 2 or 4 = a strip of 32 or 64 weight rows)
  unsigned gx, gy;
};

// -2 for a shape outside the contract or past one launch in the form chosen; then -1 for a form that is none of 0, 1, 2
inline int plan(long long M, long long E, long long N, long long K, int form, Plan* p) {
  if (M < 1 || E < 1 || N < 8 || N % 8 || K < kMx || K % kMx) return CLN_ERR_UNSUPPORTED;
  if (M > 0x7fffffffLL || E > 0x7fffffffLL - 1 || N > 0x7fffffffLL - 256 || K > 0x3fffffffLL) return CLN_ERR_UNSUPPORTED;
  const int rc = g8o::plan_form(M, E, form, &p->tile, &p->gy);
  if (rc == CLN_ERR_UNSUPPORTED) return rc;
  if (p->tile) {
    p->waves = 4;
    p->gx = (unsigned)((N + kTileN - 1) / kTileN);
  } else {
    // 64-row strips only where strips x E workgroups still give every CU one (the host cannot know how many experts are empty)
    p->waves = (N + 63) / 64 * E >= gx4::kCUs ? 4 : 2;
    p->gx = (unsigned)((N + 16 * p->waves - 1) / (16 * p->waves));
  }
  return rc;
}

inline int launch(const Args& g, const Plan& p, hipStream_t stream) {
  const dim3 grid(p.gx, p.gy), block(64 * p.waves);
  if (p.tile) CLN_LAUNCH(gemm_mxfp4_grouped_tile_mfma, grid, block, 0, stream, g);
  else CLN_LAUNCH(gemm_mxfp4_grouped_skinny_mfma, grid, block, 0, stream, g);
  return cln_check_launch();
}

}  // namespace gx4g
