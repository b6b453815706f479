// Compile unit of the bf16 packed variable-length append to a paged latent cache (multi-head latent attention): cln_kv_append_paged_mla_bf16 /
// cln_kv_append_paged_mla_bf16_describe (include/cln_amd_ext.h; kernel: kv_append_paged_mla_bf16.cuh). The checks are
// paged::mla_append_args, then paged::mla_append_shape: -1 for a missing, misaligned or aliased pointer, a non-positive dimension, a rotation
// without a table or max_pos, a table without a rotation, q without q_out; -2 for another page, rope_mode, max_pages page >= 2^31 or a grid
// that does not fit. Unlike kv_append_paged_varlen_bf16.hip, rope_mode 0 takes q and q_out: the query rows are then copied bit for bit.
#include "kv_append_paged_mla_bf16.cuh"
#include "paged_entry.h"

static_assert(kva::kMlaDc == paged::kMlaDc && kva::kMlaDr == paged::kMlaDr, "paged::mla_append_shape counts this kernel's pieces");

CLN_API int cln_kv_append_paged_mla_bf16(const void* c_new, const void* k_pe_new, void* pool, const int* block_table, const int* seqlens,
                                         const int* cu_q, const void* q, void* q_out, const float* rope_table, int B, int total_q, int Hq, int P,
                                         int max_pages, int page, int max_pos, int rope_mode, void* stream) {
  int rc = paged::mla_append_args(c_new, k_pe_new, pool, block_table, seqlens, cu_q, nullptr, false, q, q_out, rope_table, P, max_pos, rope_mode);
  if (rc != CLN_OK) return rc;
  int page_shift = 0;
  long long y = 0;
  rc = paged::mla_append_shape(B, total_q, Hq, max_pages, page, rope_mode, q != nullptr, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const kva::ArgsMlaBf16 a = {(const bf16_t*)c_new, (const bf16_t*)k_pe_new, (bf16_t*)pool, block_table, seqlens, cu_q, (const bf16_t*)q,
                              (bf16_t*)q_out, rope_table, B, total_q, Hq, P, max_pages, page_shift, max_pos};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_rope_mode(rope_mode, [&](auto m) { return kva::launch_mla_bf16<m()>(a, y, s); });
}

CLN_API int cln_kv_append_paged_mla_bf16_describe(int B, int total_q, int Hq, int max_pages, int page, int rope_mode, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = paged::mla_append_shape(B, total_q, Hq, max_pages, page, rope_mode, true, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  static const char* const rot[] = {"copied bit for bit", "rotated in half-split pairs (i, i + 32)", "rotated in interleaved pairs (2i, 2i + 1)"};
  const int n = snprintf(buf, len,
                         "kv_append_paged_mla_bf16_rows<ROPE=%d> B=%d total_q=%d Hq=%d page=%d: one launch, no workspace; %d x %lld workgroups of 256 "
                         "threads (a packed row x the 16-byte pieces of its latent pool row [c %d | k_pe %d] and, with q, its %d query rows of %d "
                         "dims, %d threads per row), the sequence of a row by binary search over the device-side offsets, length and table entry "
                         "through uniform loads, dims 0 ... %d copied bit for bit, the %d rotary dims of the pool row and of q %s%s, plain stores "
                         "into the pool; deterministic",
                         rope_mode, B, total_q, Hq, page, total_q, y, paged::kMlaDc, paged::kMlaDr, Hq, paged::kMlaDk,
                         paged::mla_append_pieces(rope_mode), paged::kMlaDc - 1, paged::kMlaDr, rot[rope_mode],
                         rope_mode ? " in fp32 from the cos/sin table [max_pos, 64] with one rounding at the store" : "");
  return n < len ? n : len - 1;
}
