// Compile unit of the packed variable-length append of bf16 rows to a paged latent cache in DeepSeek-V3.2's own FP8 row of 656 bytes:
// cln_kv_append_paged_mla_bf16_fp8_tile / cln_kv_append_paged_mla_bf16_fp8_tile_describe (include/cln_amd_ext.h; kernel:
// kv_append_paged_mla_bf16_fp8_tile.cuh). The checks are paged::mla_append_args without a scale pointer (the scales are
// computed here and live in the rows), then scale_pow2 (neither 0 nor 1: -1), then paged::mla_append_tile_shape: -1 for a missing,
// misaligned or aliased pointer, a non-positive dimension, a rotation without a table or max_pos, a table without a rotation, q without
// q_out; -2 for another page, rope_mode, max_pages page >= 2^31 or a grid that does not fit.
//
// Built without packed fp32 ops (_build.py EXTRA_FLAGS): no register reason here (18 / 48 / 26 VGPRs with them, 18 / 44 / 24 without, no
// spill either way) -- the new units of this family take no v_pk_*_f32 forms at all, and the flag is the same for the three of them.
#include "kv_append_paged_mla_bf16_fp8_tile.cuh"
#include "paged_entry.h"

static_assert(kva::kMlaDc == paged::kMlaDc && kva::kMlaDr == paged::kMlaDr && kva::kMlaTileRowBytes == paged::kMlaTileRowBytes &&
                  kva::kMlaTile == paged::kMlaTile,
              "paged::mla_append_tile_shape counts this kernel's threads");

CLN_API int cln_kv_append_paged_mla_bf16_fp8_tile(const void* c_new, const void* k_pe_new, void* pool, const int* block_table, const int* seqlens,
                                                  const int* cu_q, const void* q, void* q_out, const float* rope_table, int B, int total_q,
                                                  int Hq, int P, int max_pages, int page, int max_pos, int rope_mode, int scale_pow2,
                                                  void* stream) {
  int rc = paged::mla_append_args(c_new, k_pe_new, pool, block_table, seqlens, cu_q, nullptr, false, q, q_out, rope_table, P, max_pos, rope_mode);
  if (rc != CLN_OK) return rc;
  if (scale_pow2 != 0 && scale_pow2 != 1) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  rc = paged::mla_append_tile_shape(B, total_q, Hq, max_pages, page, rope_mode, q != nullptr, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const kva::ArgsMlaBf16Fp8Tile a = {(const bf16_t*)c_new, (const bf16_t*)k_pe_new, (uint8_t*)pool, block_table, seqlens, cu_q, (const bf16_t*)q,
                                     (bf16_t*)q_out, rope_table, B, total_q, Hq, P, max_pages, page_shift, max_pos, scale_pow2};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_rope_mode(rope_mode, [&](auto m) { return kva::launch_mla_bf16_fp8_tile<m()>(a, y, s); });
}

CLN_API int cln_kv_append_paged_mla_bf16_fp8_tile_describe(int B, int total_q, int Hq, int max_pages, int page, int rope_mode, int scale_pow2,
                                                           char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  if (scale_pow2 != 0 && scale_pow2 != 1) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = paged::mla_append_tile_shape(B, total_q, Hq, max_pages, page, rope_mode, true, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  static const char* const rot[] = {"copied bit for bit", "rotated in half-split pairs (i, i + 32)", "rotated in interleaved pairs (2i, 2i + 1)"};
  static const char* const qrot[] = {"copied bit for bit", "rotated alike", "rotated alike"};
  const int n = snprintf(buf, len,
                         "kv_append_paged_mla_bf16_fp8_tile_rows<ROPE=%d> B=%d total_q=%d Hq=%d page=%d scale_pow2=%d: one launch, no workspace, no "
                         "LDS, no atomics; %d x %lld workgroups of 256 threads; a pool row is %d bytes: %d e4m3fn codes of c, %d fp32 scales at "
                         "byte %d (one per %d-dim tile, per token), %d bf16 of k_pe at byte %d; per packed row one wave quantises c, 8 dims a "
                         "lane (16 bytes in, 8 bytes out), a DPP row of 16 lanes one tile: per tile in IEEE fp32 a = max(amax, 1e-4), scale = a "
                         "/ 448%s, inv = 1 / scale, code = e4m3fn rne of clamp(c inv, -448, 448), the amax by four DPP moves inside the row (the "
                         "64 lanes leave or stay together), lane 0 of a row stores the scale; behind the wave %d threads move the %d rotary dims "
                         "of k_pe, %s%s and stored as bf16, and with q %d threads per row move its %d bf16 query rows of %d dims, dims 0 ... %d "
                         "copied bit for bit, the rotary dims %s; the sequence of a row by binary search over the device-side offsets, length "
                         "and table entry through uniform loads, vector stores into the pool, every byte outside a live token's row untouched; "
                         "deterministic",
                         rope_mode, B, total_q, Hq, page, scale_pow2, total_q, y, paged::kMlaTileRowBytes, paged::kMlaDc, paged::kMlaTiles,
                         paged::kMlaDc, paged::kMlaTile, paged::kMlaDr, paged::kMlaDc + 4 * paged::kMlaTiles,
                         scale_pow2 ? " rounded up to a power of two on its bits (ue8m0)" : "", rope_mode == 1 ? paged::kMlaDr / 16 : paged::kMlaDr / 8,
                         paged::kMlaDr, rot[rope_mode], rope_mode ? " in fp32 from the cos/sin table [max_pos, 64] with one rounding" : "",
                         paged::mla_append_pieces(rope_mode), Hq, paged::kMlaDk, paged::kMlaDc - 1, qrot[rope_mode]);
  return n < len ? n : len - 1;
}
