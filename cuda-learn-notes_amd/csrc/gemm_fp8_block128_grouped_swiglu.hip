// Compile unit of the fused gate/up projection of an MoE FFN: cln_gemm_fp8_block128_grouped_swiglu_fp8 /
// cln_gemm_fp8_block128_grouped_swiglu_fp8_describe (include/cln_amd_ext.h; kernels and plan: gemm_fp8_block128_grouped_swiglu.cuh; DESIGN
// 4.4.30). Status: -2 for a shape outside M_total >= 1, E >= 1, I >= 128 with I % 128 == 0, K >= 128 with K % 128 == 0 (or past one launch: E,
// or the tile form's slots, above 65535); then -1 for a missing, misaligned (a, b, h 16 bytes; the scales and the offsets 4) or aliased
// pointer, a scale_pow2 that is neither 0 nor 1, or a form that is none of 0 (by the rule), 1 (skinny), 2 (tile).
#include "gemm_fp8_block128_grouped_swiglu.cuh"

CLN_API int cln_gemm_fp8_block128_grouped_swiglu_fp8(const void* a, const float* a_scale, const void* b, const float* b_scale,
                                                     const int* expert_offsets, void* h, float* h_scale, int M_total, int E, int I, int K,
                                                     int form, int scale_pow2, void* stream) {
  g8s::Plan p;
  const int rc = g8s::plan(M_total, E, I, K, form, &p);
  if (rc == CLN_ERR_UNSUPPORTED) return rc;
  if (!a || !a_scale || !b || !b_scale || !expert_offsets || !h || !h_scale) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(a) || !cln_aligned16(b) || !cln_aligned16(h) || !cln_aligned(a_scale, 4) || !cln_aligned(b_scale, 4) ||
      !cln_aligned(expert_offsets, 4) || !cln_aligned(h_scale, 4))
    return CLN_ERR_BAD_ARG;
  auto is_input = [&](const void* out) {
    return out == a || out == b || out == (const void*)a_scale || out == (const void*)b_scale || out == (const void*)expert_offsets;
  };
  if (is_input(h) || is_input(h_scale) || (const void*)h == (const void*)h_scale) return CLN_ERR_BAD_ARG;
  if (scale_pow2 != 0 && scale_pow2 != 1) return CLN_ERR_BAD_ARG;
  if (rc != CLN_OK) return rc;  // the form
  const g8s::Args args = {(const uint8_t*)a, (const uint8_t*)b, a_scale,           b_scale, expert_offsets, (uint8_t*)h, h_scale,
                          M_total,           E,                 I,                 K / g8::kBlock, scale_pow2};
  return g8s::launch(args, p, (hipStream_t)stream);
}

// what hipcc (ROCm 7.2) reports for the two kernels: arch VGPRs + AGPRs
static void g8s_regs(const g8s::Plan& p, int* v, int* a) {
  if (p.tile) *v = 256, *a = 145;
  else *v = 249, *a = 0;
}

CLN_API int cln_gemm_fp8_block128_grouped_swiglu_fp8_describe(int M_total, int E, int I, int K, int form, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  g8s::Plan p;
  const int rc = g8s::plan(M_total, E, I, K, form, &p);
  if (rc != CLN_OK) return rc;
  int v = 0, ag = 0;
  g8s_regs(p, &v, &ag);
  char why[96];
  g8o::why_form(why, sizeof why, M_total, E, form, p.tile);
  const long long slots = (long long)M_total / g8::kTileM + E;
  int n;
  if (p.tile)
    n = snprintf(buf, len,
                 "gemm_fp8_block128_grouped_swiglu_tile_mfma M_total=%d E=%d I=%d K=%d: form tile (%s), one launch, expert offsets read on the "
                 "device (clamped to [0, M_total]), no workspace, no atomics, 0 bytes scratch; grid %u x %u workgroups of 256 threads (4 "
                 "waves): %u column tiles of h x %lld slots = floor(M_total / %d) + E, expert e owns the slots from floor(off[e] / %d) + e, found "
                 "by binary search over the offsets (scalar loads); a workgroup owns %d rows x %d columns of h = the gate tile and the up tile "
                 "of the same columns (weight rows n and I + n, scale blocks t and I / 128 + t); rows clamped on load to the expert's own last "
                 "row, stores masked at the expert's end; per K block of 128 32 v_mfma_f32_16x16x128_f8f6f4 a wave from 8 weight and 4 "
                 "activation fragment reads (weights = SrcA, activations = SrcB, zero C, e4m3 both, no hardware scale), then s = sa * sb (two sb "
                 "a block, scalar loads) and 4 fmaf per sub-tile into 128 fp32 master accumulators (G and U, never rounded to bf16); %d K "
                 "blocks through a ring of 2 LDS slots of %d bytes (256 weight rows, 128 activation rows, their sa), %d bytes dynamic, filled "
                 "through registers, 16-byte chunk c of row r at c ^ ((r >> 1) & 7); one barrier a K block; epilogue in registers: hf = G * "
                 "rcp(1 + exp(-G)) * U (v_exp_f32, v_rcp_f32; G >= 32 gives G), row amax over the lane's 16 values, the 4 lane groups "
                 "(permlane swaps) and the 2 waves of a row (1024 bytes of the free ring, one barrier), scale = max(amax, 1e-4) / 448, "
                 "code = e4m3fn rne of clamp(hf * (1 / scale), +-448): one 4-byte code store a lane and sub-tile, one float a row; %d VGPRs + "
                 "%d AGPRs, no spill; 64-bit element offsets; deterministic",
                 M_total, E, I, K, why, p.gx, p.gy, p.gx, slots, g8::kTileM, g8::kTileM, g8::kTileM, g8::kTileN, K / g8::kBlock, g8s::kSlotBytes,
                 g8s::kTileLds, v, ag);
  else
    n = snprintf(buf, len,
                 "gemm_fp8_block128_grouped_swiglu_skinny_mfma M_total=%d E=%d I=%d K=%d: form skinny (%s), one launch, expert offsets read on "
                 "the device (clamped to [0, M_total]), no workspace, no atomics, 0 bytes scratch; grid %u x %u workgroups of %d threads (%d "
                 "waves): %u column blocks of h x E experts; wave w owns the gate rows 128 t + 16 w ... and the up rows I + the same; "
                 "empty-expert exit: a workgroup reads off[e], off[e + 1] by scalar loads and returns before its first weight load when M_e = 0; "
                 "else it walks the expert's rows in chunks of up to %d, MT = 1, 2 or 4 sub-tiles of 16 rows by the rows left (workgroup-uniform); "
                 "weights from global memory straight into the MFMA operand registers, two rings (gate, up) of %d K blocks in registers, every "
                 "weight byte read by exactly one wave; activations and their scales to registers one K block ahead; per K block of 128 2 MT "
                 "v_mfma_f32_16x16x128_f8f6f4 a wave (weights = SrcA, activations = SrcB, zero C, e4m3 both, no hardware scale), then s = sa * sb "
                 "(two sb a block, scalar loads) and 4 fmaf per sub-tile into fp32 master accumulators (G and U, never rounded to bf16); %d K "
                 "blocks, no split over K; per chunk hf = G * rcp(1 + exp(-G)) * U in registers (v_exp_f32, v_rcp_f32; G >= 32 gives G), each "
                 "wave's 16-column amax of a row over the 4 lane groups (permlane swaps), then over the 8 waves through LDS (%d bytes static, "
                 "two buffers by the chunk's parity, one barrier a chunk); scale = max(amax, 1e-4) / 448, code = e4m3fn rne of clamp(hf * (1 / "
                 "scale), +-448): one 4-byte code store a lane, one float a row; rows clamped on load, masked on store at the chunk's end; %d "
                 "VGPRs + %d AGPRs, no spill; 64-bit element offsets; deterministic; the tile form would use %lld slots",
                 M_total, E, I, K, why, p.gx, p.gy, g8s::kSkinnyThreads, g8s::kSkinnyWaves, p.gx, g8s::kChunk, g8::kPF, K / g8::kBlock,
                 g8s::kSkinnyLds, v, ag, slots);
  return n < len ? n : len - 1;
}
