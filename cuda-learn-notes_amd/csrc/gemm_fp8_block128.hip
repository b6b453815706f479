// Compile unit of the block-scaled FP8 GEMM: cln_gemm_fp8_block128_bf16 / cln_gemm_fp8_block128_bf16_describe (include/cln_amd_ext.h; kernel and
// plan: gemm_fp8_block128.cuh). Status: -2 for a shape outside M >= 1, N >= 8 with N % 8 == 0, K >= 128 with K % 128 == 0 (or past
// one launch); then -1 for a missing, misaligned (a, b, out 16 bytes; the scales 4) or aliased pointer.
#include "gemm_fp8_block128.cuh"

CLN_API int cln_gemm_fp8_block128_bf16(const void* a, const float* a_scale, const void* b, const float* b_scale, void* out, int M, int N, int K,
                                       void* stream) {
  g8::Plan p;
  const int rc = g8::plan(M, N, K, &p);
  if (rc != CLN_OK) return rc;
  if (!a || !a_scale || !b || !b_scale || !out) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(a) || !cln_aligned16(b) || !cln_aligned16(out) || !cln_aligned(a_scale, 4) || !cln_aligned(b_scale, 4)) return CLN_ERR_BAD_ARG;
  if (out == a || out == b || out == (const void*)a_scale || out == (const void*)b_scale) return CLN_ERR_BAD_ARG;
  const g8::Args args = {(const uint8_t*)a, (const uint8_t*)b, a_scale, b_scale, (bf16_t*)out, M, N, K / g8::kBlock};
  return g8::launch(args, p, (hipStream_t)stream);
}

// what hipcc (ROCm 7.2) reports for the four instantiations: arch VGPRs + AGPRs (the AGPRs are the MFMA results on their way to the fmaf)
static void g8_regs(const g8::Plan& p, int* v, int* a) {
  if (p.tile) *v = 190, *a = 64;
  else if (p.mt == 1) *v = 82, *a = 4;
  else if (p.mt == 2) *v = 120, *a = 8;
  else *v = 190, *a = 16;
}

CLN_API int cln_gemm_fp8_block128_bf16_describe(int M, int N, int K, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  g8::Plan p;
  const int rc = g8::plan(M, N, K, &p);
  if (rc != CLN_OK) return rc;
  int v = 0, ag = 0;
  g8_regs(p, &v, &ag);
  int n;
  if (p.tile)
    n = snprintf(buf, len,
                 "gemm_fp8_block128_mfma<tile> M=%d N=%d K=%d: form tile (M > %d), one launch, no workspace, no atomics, 0 bytes scratch; grid %u x "
                 "%u workgroups of 256 threads (4 waves), output tile %d (m) x %d (n), a wave owns 64 x 64 = 4 x 4 sub-tiles; per K block of 128 "
                 "16 v_mfma_f32_16x16x128_f8f6f4 a wave (weights = SrcA, activations = SrcB, zero C, e4m3 both, no hardware scale), then s = sa * "
                 "sb and 4 fmaf per sub-tile into 64 fp32 master accumulators; %d K blocks through a ring of 2 LDS slots of %d bytes (128 x 128 "
                 "weight codes, 128 x 128 activation codes, 128 sa), %d bytes static, filled through registers, 16-byte chunk c of row r at c ^ "
                 "((r >> 1) & 7); one barrier a K block; edge rows clamped on load, masked on store; %d VGPRs + %d AGPRs, no spill; one bf16 x 4 "
                 "store a lane and sub-tile; deterministic",
                 M, N, K, g8::kSkinnyMaxM, p.gx, p.gy, g8::kTileM, g8::kTileN, K / g8::kBlock, g8::kSlotBytes, g8::kTileLds, v, ag);
  else
    n = snprintf(buf, len,
                 "gemm_fp8_block128_mfma<skinny, MT=%d> M=%d N=%d K=%d: form skinny (M <= %d), one launch, no workspace, no atomics, no LDS, 0 bytes "
                 "scratch; grid %u workgroups of %d threads (%d waves): a strip of %d weight rows (a wave 16) x all of M padded to %d rows; "
                 "weights from global memory straight into the MFMA operand registers (32 bytes a lane, two 16-byte loads), a ring of %d K blocks "
                 "in registers; activations and their scales to registers one K block ahead; per K block of 128 %d "
                 "v_mfma_f32_16x16x128_f8f6f4 a wave (weights = SrcA, activations = SrcB, zero C, e4m3 both, no hardware scale), then s = sa * sb "
                 "and 4 fmaf per sub-tile into fp32 master accumulators; %d K blocks, no split over K; rows clamped on load, masked on store; %d "
                 "VGPRs + %d AGPRs, no spill; one bf16 x 4 store a lane and sub-tile; deterministic",
                 p.mt, M, N, K, g8::kSkinnyMaxM, p.gx, 64 * p.waves, p.waves, 16 * p.waves, 16 * p.mt, g8::kPF, p.mt, K / g8::kBlock, v, ag);
  return n < len ? n : len - 1;
}
