// Compile unit of the grouped (MoE) MXFP4-weight GEMM: cln_gemm_mxfp4_grouped_bf16 / cln_gemm_mxfp4_grouped_bf16_describe
// (include/cln_amd_ext.h; kernels and plan: gemm_mxfp4_grouped.cuh). Status: -2 for a shape outside M_total >= 1, E >= 1, N >= 8
// with N % 8 == 0, K >= 32 with K % 32 == 0 (or past one launch: E, or the tile form's slots, above 65535); then -1 for a missing, misaligned
// (a, b, out, bias 16 bytes; the offsets 4) or aliased pointer, or a form that is none of 0 (by the rule), 1 (skinny), 2 (tile).
#include "gemm_mxfp4_grouped.cuh"

CLN_API int cln_gemm_mxfp4_grouped_bf16(const void* a, const void* a_scale, const void* b, const void* b_scale, const void* bias,
                                        const int* expert_offsets, void* out, int M_total, int E, int N, int K, int form, void* stream) {
  gx4g::Plan p;
  const int rc = gx4g::plan(M_total, E, N, K, form, &p);
  if (rc == CLN_ERR_UNSUPPORTED) return rc;
  if (!a || !a_scale || !b || !b_scale || !expert_offsets || !out) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(a) || !cln_aligned16(b) || !cln_aligned16(out) || !cln_aligned16(bias) || !cln_aligned(expert_offsets, 4)) return CLN_ERR_BAD_ARG;
  if (out == a || out == b || out == a_scale || out == b_scale || out == bias || out == (const void*)expert_offsets) return CLN_ERR_BAD_ARG;
  if (rc != CLN_OK) return rc;  // the form
  const gx4g::Args args = {(const uint8_t*)a, (const uint8_t*)b, (const uint8_t*)a_scale, (const uint8_t*)b_scale, (const bf16_t*)bias,
                           expert_offsets, (bf16_t*)out, M_total, E, N, K};
  return gx4g::launch(args, p, (hipStream_t)stream);
}

// what hipcc (ROCm 7.2) reports for the two kernels: arch VGPRs + AGPRs (the skinny kernel holds gx4::skinny<1>, <2> and <4>: the largest counts)
static void gx4g_regs(const gx4g::Plan& p, int* v, int* a) {
  if (p.tile) *v = 107, *a = 64;
  else *v = 218, *a = 16;
}

CLN_API int cln_gemm_mxfp4_grouped_bf16_describe(int M_total, int E, int N, int K, int form, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  gx4g::Plan p;
  const int rc = gx4g::plan(M_total, E, N, K, form, &p);
  if (rc != CLN_OK) return rc;
  int v = 0, ag = 0;
  gx4g_regs(p, &v, &ag);
  char why[96];
  g8o::why_form(why, sizeof why, M_total, E, form, p.tile);
  const int KS = (K + gx4::kStep - 1) / gx4::kStep;
  int n;
  if (p.tile)
    n = snprintf(buf, len,
                 "gemm_mxfp4_grouped_tile_mfma M_total=%d E=%d N=%d K=%d: form tile (%s), one launch, expert offsets read on the device (clamped "
                 "to [0, M_total]), no workspace, no atomics, 0 bytes scratch; grid %u x %u workgroups of 256 threads (4 waves): %u N tiles x %u "
                 "slots = floor(M_total / %d) + E, expert e owns the slots from floor(off[e] / %d) + e; a workgroup finds its expert by binary "
                 "search over the offsets (scalar loads) and exits when its slot lies behind the expert's last tile (at most E empty slots; an "
                 "empty expert owns none); output tile %d (m) x %d (n) from the expert's own first row, rows clamped on load to the expert's own "
                 "last row, stores masked at the expert's end; per K step of 128 16 v_mfma_scale_f32_16x16x128_f8f6f4 a wave (weights = SrcA e2m1 "
                 "in 4 VGPRs, activations = SrcB e4m3, each lane its own two e8m0 scale bytes, op_sel 0), the 64 fp32 accumulators chained "
                 "through the C operand from the expert's bias on: no fp32 work in the loop; %d K steps (a slice at or beyond K feeds a zero "
                 "weight operand) through a ring of 2 LDS slots of %d bytes, %d bytes static, filled through registers, 16-byte weight chunk c "
                 "of row r at c ^ ((r >> 2) & 3), activation chunk c at c ^ ((r >> 1) & 7); one barrier a K step; %d VGPRs + %d AGPRs, no "
                 "spill; 64-bit element offsets; deterministic: an expert's rows carry the bits of gemm_mxfp4_bf16 on that expert alone",
                 M_total, E, N, K, why, p.gx, p.gy, p.gx, p.gy, gx4::kTileM, gx4::kTileM, gx4::kTileM, gx4::kTileN, KS, gx4::kSlotBytes,
                 gx4::kTileLds, v, ag);
  else
    n = snprintf(buf, len,
                 "gemm_mxfp4_grouped_skinny_mfma M_total=%d E=%d N=%d K=%d: form skinny (%s), one launch, expert offsets read on the device "
                 "(clamped to [0, M_total]), no workspace, no atomics, no LDS, 0 bytes scratch; grid %u x %u workgroups of %d threads (%d "
                 "waves): %u strips of %d weight rows (a wave 16; 64-row strips where strips x E >= %d) x E experts; empty-expert exit: a "
                 "workgroup reads off[e], off[e + 1] by scalar loads and returns before its first weight load when M_e = 0; else it walks the "
                 "expert's rows in chunks of up to 64, MT = 1, 2 or 4 sub-tiles of 16 rows by the rows left (workgroup-uniform); weight nibbles "
                 "from global memory straight into the four MFMA operand registers (16 bytes a lane and K step, one load), a ring of %d K steps "
                 "in registers with their scale bytes; activations and their scale bytes to registers one K step ahead; per K step of 128 MT "
                 "v_mfma_scale_f32_16x16x128_f8f6f4 a wave (weights = SrcA e2m1 in 4 VGPRs, activations = SrcB e4m3, each lane its own two e8m0 "
                 "scale bytes, op_sel 0), the fp32 accumulators chained through the C operand from the expert's bias on: no fp32 work in the "
                 "loop; %d K steps (a slice at or beyond K feeds a zero weight operand), no split over K; rows clamped on load, masked on "
                 "store at the chunk's end; %d VGPRs + %d AGPRs, no spill; 64-bit element offsets; deterministic: an expert's rows carry the "
                 "bits of gemm_mxfp4_bf16 on that expert alone; the tile form would use %lld slots",
                 M_total, E, N, K, why, p.gx, p.gy, 64 * p.waves, p.waves, p.gx, 16 * p.waves, gx4::kCUs, gx4::kPF, KS, v, ag,
                 (long long)M_total / gx4::kTileM + E);
  return n < len ? n : len - 1;
}
