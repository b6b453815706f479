// Grouped (mixture-of-experts) block-scaled FP8 GEMM over expert offsets that live on the device (cln_gemm_fp8_block128_grouped_bf16,
// include/cln_amd_ext.h): the rows of a [M_total, K] are sorted by expert, expert e owns the rows off[e] ... off[e + 1] - 1 and
// its own weight b[e] [N, K] with its own scale grid b_scale[e] [ceil(N/128), K/128]; for a row m of expert e
//   out[m, n] = bf16_rne( sum_kb  a_scale[m, kb] * b_scale[e, n / 128, kb] * sum_{k in block kb} fp32(a[m, k]) * fp32(b[e, n, k]) )
// This header owns the two grouped kernels, the view of one expert, the plan and the launch. Both bodies are the dense form's
// (gemm_fp8_block128_core.cuh: g8::skinny<MT>, g8::tile) called on a view of the expert, so the arithmetic of an element -- one
// v_mfma_f32_16x16x128_f8f6f4 per scale block with a zero C operand, s = sa * sb, fmaf in ascending kb, one rounding -- is the dense entry's,
// and an expert's rows carry the bits the dense entry gives on that expert alone, in either form. How the work is found and split when the
// host cannot see the offsets -- the clamp, the slots, the search, the form rule -- is gemm_fp8_block128_offsets.cuh's (g8o).
//
// SKINNY (decode: few rows an expert, bound by weight bytes). Grid (strips of 32 or 64 weight rows) x E: workgroup (x, e) owns strip x of
// expert e's weight and ALL of the expert's rows, and returns before its first weight load when M_e = 0. Otherwise it walks the expert's rows
// in chunks of up to 64; per chunk the 16-row sub-tile count MT in {1, 2, 4} comes from the rows left (a workgroup-uniform branch over
// g8::skinny's three instantiations, called on a view of the expert: the chunk's rows as M, the expert's weight and scale grid as b, sb).
// No LDS, no barrier. A second chunk re-reads the strip (32 or 64 x K bytes, from L2): the form is for experts of at most a few chunks, the
// rule sends longer groups to the tile form.
//
// TILE (prefill: compute-bound). Tiles of 128 x 128, N tiles in x, the slots of g8o in y. The body is g8::tile on a view of the expert
// (M = M_e) with the tile's first row 128 t relative to the expert: row indices are clamped on load to the expert's OWN last row and stores
// are masked at the expert's end, not at M_total -- the next expert's rows belong to another workgroup with other weights. sb comes from the
// expert's own grid, one scalar load a K block.
//
// Element offsets are 64-bit, e N K included (256 x 4096 x 7168 is 7.5e9 bytes). One launch, nothing read on the host, no workspace, no
// atomics; deterministic; graph-capturable with the offsets changing between replays. cln_mfma_keep stands behind every MFMA (inside
// g8::mfma128). The unit is built without packed fp32 ops (_build.py), and this file writes none.
#pragma once
#include "gemm_fp8_block128_core.cuh"
#include "gemm_fp8_block128_offsets.cuh"

namespace g8g {

using g8::kBlock;
using g8::kTileM;
using g8::kTileN;

struct Args {
  const uint8_t *a, *b;  // [M,K], [E,N,K] e4m3fn
  const float *sa, *sb;  // [M,KB], [E,NB,KB]
  const int* off;        // [E + 1], on the device
  bf16_t* out;           // [M,N]
  int M, E, N, KB;       // M = M_total, KB = K / 128
};

// The dense kernel's arguments on expert e alone: its weight, its scale grid, and its rows from row c0 + m0 on, `rows` of them.
__device__ __forceinline__ g8::Args expert_view(const Args& g, int e, int c0, int m0, int rows) {
  const size_t r0 = (size_t)c0 + (size_t)m0, NB = (size_t)((g.N + kBlock - 1) / kBlock);
  const size_t ldk = (size_t)g.KB * kBlock;
  return {g.a + r0 * ldk, g.b + (size_t)e * (size_t)g.N * ldk, g.sa + r0 * g.KB, g.sb + (size_t)e * NB * g.KB, g.out + r0 * g.N, rows, g.N, g.KB};
}

// ---- the skinny form: grid (strips, E), blockDim.x = 64 W
__global__ __launch_bounds__(256) void gemm_fp8_block128_grouped_skinny_mfma(const Args g) {
  const int e = blockIdx.y;
  const g8o::Rows r = g8o::expert_rows(g.off, g.M, e);
  if (r.Me == 0) return;  // the empty-expert exit: nothing of b[e] has been addressed
  for (int m0 = 0; m0 < r.Me; m0 += 64) {
    const int rows = min(64, r.Me - m0);
    const g8::Args d = expert_view(g, e, r.c0, m0, rows);
    if (rows <= 16) g8::skinny<1>(d);
    else if (rows <= 32) g8::skinny<2>(d);
    else g8::skinny<4>(d);
  }
}

// ---- the tile form: grid (N tiles, slots)
__global__ __launch_bounds__(256) void gemm_fp8_block128_grouped_tile_mfma(const Args g) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[g8::kTileLds];
  g8o::Tile w;
  if (!g8o::tile_of_slot(g.off, g.M, g.E, blockIdx.y, &w)) return;  // uniform, before any barrier
  g8::tile(expert_view(g, w.e, w.c0, 0, w.Me), kTileM * w.t, smem);  // masked at the view's M = the expert's end
}

// ---- the plan: a function of (M_total, E, N, K, form) only (the entry and its describe share it)
struct Plan {
  int tile;   // 1: the tile form
  int waves;  // waves a workgroup (skinny: 2 or 4 = a strip of 32 or 64 weight rows)
  unsigned gx, gy;
};

// -2 for a shape outside the contract or past one launch in the form chosen; then -1 for a form that is none of 0, 1, 2
inline int plan(long long M, long long E, long long N, long long K, int form, Plan* p) {
  if (M < 1 || E < 1 || N < 8 || N % 8 || K < kBlock || K % kBlock) return CLN_ERR_UNSUPPORTED;
  if (M > 0x7fffffffLL || E > 0x7fffffffLL - 1 || N > 0x7fffffffLL - 256 || K > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  const int rc = g8o::plan_form(M, E, form, &p->tile, &p->gy);
  if (rc == CLN_ERR_UNSUPPORTED) return rc;
  if (p->tile) {
    p->waves = 4;
    p->gx = (unsigned)((N + kTileN - 1) / kTileN);
  } else {
    // 64-row strips only where strips x E workgroups still give every CU one (the host cannot know how many experts are empty)
    p->waves = (N + 63) / 64 * E >= g8::kCUs ? 4 : 2;
    p->gx = (unsigned)((N + 16 * p->waves - 1) / (16 * p->waves));
  }
  return rc;
}

inline int launch(const Args& g, const Plan& p, hipStream_t stream) {
  const dim3 grid(p.gx, p.gy), block(64 * p.waves);
  if (p.tile) CLN_LAUNCH(gemm_fp8_block128_grouped_tile_mfma, grid, block, 0, stream, g);
  else CLN_LAUNCH(gemm_fp8_block128_grouped_skinny_mfma, grid, block, 0, stream, g);
  return cln_check_launch();
}

}  // namespace g8g
