// Compile unit of the MXFP4-weight GEMM: cln_gemm_mxfp4_bf16 / cln_gemm_mxfp4_bf16_describe (include/cln_amd_ext.h; kernel and plan:
// gemm_mxfp4.cuh). Status: -2 for a shape outside M >= 1, N >= 8 with N % 8 == 0, K >= 32 with K % 32 == 0 (or past one launch);
// then -1 for a missing, misaligned (a, b, out, bias 16 bytes) or aliased pointer, or a form that is none of 0 (by the rule), 1 (skinny), 2 (tile).
#include "gemm_mxfp4.cuh"

CLN_API int cln_gemm_mxfp4_bf16(const void* a, const void* a_scale, const void* b, const void* b_scale, const void* bias, void* out, int M, int N,
                                int K, int form, void* stream) {
  gx4::Plan p;
  const int rc = gx4::plan(M, N, K, form, &p);
  if (rc == CLN_ERR_UNSUPPORTED) return rc;
  if (!a || !a_scale || !b || !b_scale || !out) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(a) || !cln_aligned16(b) || !cln_aligned16(out) || !cln_aligned16(bias)) return CLN_ERR_BAD_ARG;
  if (out == a || out == b || out == a_scale || out == b_scale || out == bias) return CLN_ERR_BAD_ARG;
  if (rc != CLN_OK) return rc;  // the form
  const gx4::Args args = {(const uint8_t*)a, (const uint8_t*)b, (const uint8_t*)a_scale, (const uint8_t*)b_scale, (const bf16_t*)bias, (bf16_t*)out, M, N, K};
  return gx4::launch(args, p, (hipStream_t)stream);
}

// what hipcc (ROCm 7.2) reports for the four instantiations: arch VGPRs + AGPRs
static void gx4_regs(const gx4::Plan& p, int* v, int* a) {
  if (p.tile) *v = 107, *a = 64;
  else if (p.mt == 1) *v = 127, *a = 4;
  else if (p.mt == 2) *v = 164, *a = 8;
  else *v = 212, *a = 16;
}

CLN_API int cln_gemm_mxfp4_bf16_describe(int M, int N, int K, int form, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  gx4::Plan p;
  const int rc = gx4::plan(M, N, K, form, &p);
  if (rc != CLN_OK) return rc;
  int v = 0, ag = 0;
  gx4_regs(p, &v, &ag);
  char why[96];
  if (form == g8o::kAuto) snprintf(why, sizeof why, "by the rule: M %s %d", p.tile ? ">" : "<=", gx4::kSkinnyMaxM);
  else snprintf(why, sizeof why, "pinned; the rule gives %s", M <= gx4::kSkinnyMaxM ? "skinny" : "tile");
  const int KS = (K + gx4::kStep - 1) / gx4::kStep;
  int n;
  if (p.tile)
    n = snprintf(buf, len,
                 "gemm_mxfp4_mfma<tile> M=%d N=%d K=%d: form tile (%s), one launch, no workspace, no atomics, 0 bytes scratch; grid %u x %u "
                 "workgroups of 256 threads (4 waves), output tile %d (m) x %d (n), a wave owns 64 x 64 = 4 x 4 sub-tiles; per K step of 128 16 "
                 "v_mfma_scale_f32_16x16x128_f8f6f4 a wave (weights = SrcA e2m1 in 4 VGPRs, activations = SrcB e4m3, each lane its own two e8m0 "
                 "scale bytes, op_sel 0), the 64 fp32 accumulators chained through the C operand from the bias on: no fp32 work in the loop; %d K "
                 "steps (a slice at or beyond K feeds a zero weight operand) through a ring of 2 LDS slots of %d bytes (128 x 64 weight nibbles, "
                 "128 x 128 activation codes, 2 x 128 x 4 scale bytes), %d bytes static, filled through registers, 16-byte weight chunk c of row "
                 "r at c ^ ((r >> 2) & 3), activation chunk c at c ^ ((r >> 1) & 7); one barrier a K step; edge rows clamped on load, masked on "
                 "store; %d VGPRs + %d AGPRs, no spill; one bf16 x 4 store a lane and sub-tile; deterministic",
                 M, N, K, why, p.gx, p.gy, gx4::kTileM, gx4::kTileN, KS, gx4::kSlotBytes, gx4::kTileLds, v, ag);
  else
    n = snprintf(buf, len,
                 "gemm_mxfp4_mfma<skinny, MT=%d> M=%d N=%d K=%d: form skinny (%s), one launch, no workspace, no atomics, no LDS, 0 bytes scratch; "
                 "grid %u workgroups of %d threads (%d waves): a strip of %d weight rows (a wave 16) x all of M in chunks of %d rows; weight "
                 "nibbles from global memory straight into the four MFMA operand registers (16 bytes a lane and K step, one load), a ring of %d "
                 "K steps in registers with their scale bytes; activations and their scale bytes to registers one K step ahead; per K step of "
                 "128 %d v_mfma_scale_f32_16x16x128_f8f6f4 a wave (weights = SrcA e2m1 in 4 VGPRs, activations = SrcB e4m3, each lane its own two "
                 "e8m0 scale bytes, op_sel 0), the fp32 accumulators chained through the C operand from the bias on: no fp32 work in the loop; %d "
                 "K steps (a slice at or beyond K feeds a zero weight operand), no split over K; rows clamped on load, masked on store; %d VGPRs "
                 "+ %d AGPRs, no spill; one bf16 x 4 store a lane and sub-tile; deterministic",
                 p.mt, M, N, K, why, p.gx, 64 * p.waves, p.waves, 16 * p.waves, 16 * p.mt, gx4::kPF, p.mt, KS, v, ag);
  return n < len ? n : len - 1;
}
