// Compile unit of the packed variable-length append of bf16 rows to a paged latent cache held in FP8 (multi-head latent attention):
// cln_kv_append_paged_mla_bf16_fp8 / cln_kv_append_paged_mla_bf16_fp8_describe (include/cln_amd_ext.h; kernel: kv_append_paged_mla_bf16_fp8.cuh;
// DESIGN 4.4.19). The checks are paged::mla_append_args with kv_scale (fp32 [1] on the device, behind cu_q) required, then paged::mla_append_shape: -1 for a
// missing, misaligned or aliased pointer, a non-positive dimension, a rotation without a table or max_pos, a table without a rotation, q without
// q_out; -2 for another page, rope_mode, max_pages page >= 2^31 or a grid that does not fit.
#include "kv_append_paged_mla_bf16_fp8.cuh"
#include "paged_entry.h"

static_assert(kva::kMlaDc == paged::kMlaDc && kva::kMlaDr == paged::kMlaDr, "paged::mla_append_shape counts this kernel's pieces");

CLN_API int cln_kv_append_paged_mla_bf16_fp8(const void* c_new, const void* k_pe_new, void* pool, const int* block_table, const int* seqlens,
                                             const int* cu_q, const float* kv_scale, const void* q, void* q_out, const float* rope_table, int B,
                                             int total_q, int Hq, int P, int max_pages, int page, int max_pos, int rope_mode, void* stream) {
  int rc = paged::mla_append_args(c_new, k_pe_new, pool, block_table, seqlens, cu_q, kv_scale, true, q, q_out, rope_table, P, max_pos, rope_mode);
  if (rc != CLN_OK) return rc;
  int page_shift = 0;
  long long y = 0;
  rc = paged::mla_append_shape(B, total_q, Hq, max_pages, page, rope_mode, q != nullptr, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const kva::ArgsMlaBf16Fp8 a = {(const bf16_t*)c_new, (const bf16_t*)k_pe_new, (uint8_t*)pool, block_table, seqlens, cu_q, kv_scale,
                                 (const bf16_t*)q, (bf16_t*)q_out, rope_table, B, total_q, Hq, P, max_pages, page_shift, max_pos};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_rope_mode(rope_mode, [&](auto m) { return kva::launch_mla_bf16_fp8<m()>(a, y, s); });
}

CLN_API int cln_kv_append_paged_mla_bf16_fp8_describe(int B, int total_q, int Hq, int max_pages, int page, int rope_mode, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = paged::mla_append_shape(B, total_q, Hq, max_pages, page, rope_mode, true, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  static const char* const rot[] = {"quantised as they are", "rotated in half-split pairs (i, i + 32)", "rotated in interleaved pairs (2i, 2i + 1)"};
  static const char* const qrot[] = {"copied bit for bit", "rotated alike", "rotated alike"};
  const int n = snprintf(buf, len,
                         "kv_append_paged_mla_bf16_fp8_rows<ROPE=%d> B=%d total_q=%d Hq=%d page=%d: one launch, no workspace; %d x %lld workgroups of "
                         "256 threads (a packed row x the 8-element pieces of its latent pool row [c %d | k_pe %d] of e4m3fn codes and, with q, its "
                         "%d bf16 query rows of %d dims, %d threads per row), the sequence of a row by binary search over the device-side offsets, "
                         "length and table entry through uniform loads, the pool row quantised per element in fp32 as e4m3(clamp(y (1 / kv_scale), "
                         "+-448)), round to nearest even (v_cvt_pk_fp8_f32), kv_scale fp32 [1] on the device, so that a stored byte means the code "
                         "(v_cvt_scalef32_pk_bf16_fp8, exact) times kv_scale; dims 0 ... %d from the bf16 input, the %d rotary dims of the pool row "
                         "%s%s, those of q %s and stored as bf16, dims 0 ... %d of q copied bit for bit, plain stores into the pool; deterministic",
                         rope_mode, B, total_q, Hq, page, total_q, y, paged::kMlaDc, paged::kMlaDr, Hq, paged::kMlaDk,
                         paged::mla_append_pieces(rope_mode), paged::kMlaDc - 1, paged::kMlaDr, rot[rope_mode],
                         rope_mode ? " in fp32 from the cos/sin table [max_pos, 64] with no bf16 rounding in front of the quantiser" : "",
                         qrot[rope_mode], paged::kMlaDc - 1);
  return n < len ? n : len - 1;
}
