// Compile unit of the bf16 packed variable-length paged KV-cache append entries at head dim 256: cln_kv_append_paged_varlen_d256_bf16 /
// cln_kv_append_paged_varlen_d256_bf16_describe (include/cln_amd_ext.h). The kernel is kva::kv_append_paged_varlen_bf16_rows
// (kv_append_paged_varlen_bf16.cuh) instantiated at D = 256: its body names D only through the threads per row (D / 16 with the half-split
// pairs (i, i + D/2) = (i, i + 128), which one thread reads and writes as two 16-byte pieces; D / 8 otherwise), the row strides and the table
// row [cos D/2 | sin D/2], and kva::grid_y counts the same pieces. The checks and the status codes are those of kv_append_paged_varlen_bf16.hip
// with paged::append_shape_d256 in place of paged::append_shape: D = 256 only.
#include "kv_append_paged_varlen_bf16.cuh"
#include "paged_entry.h"

CLN_API int cln_kv_append_paged_varlen_d256_bf16(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table,
                                                 const int* seqlens, const int* cu_q, const void* q, void* q_out, const float* rope_table, int B,
                                                 int total_q, int Hq, int Hkv, int P, int max_pages, int page, int D, int max_pos, int rope_mode,
                                                 void* stream) {
  const void* const in[] = {k_new, v_new, block_table, seqlens, cu_q, q, rope_table};  // the required inputs, then q and rope_table
  const int al4[] = {0, 0, 1, 1, 1, 0, 1};
  int rc = paged::append_args(in, al4, 5, {k_pages, v_pages, q_out}, P, max_pos, rope_mode);
  if (rc != CLN_OK) return rc;
  int page_shift = 0;
  long long y = 0;
  rc = paged::append_shape_d256(true, B, total_q, Hq, Hkv, max_pages, page, D, rope_mode, q != nullptr, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const kva::ArgsVarlenBf16 a = {(const bf16_t*)k_new, (const bf16_t*)v_new, (bf16_t*)k_pages, (bf16_t*)v_pages, block_table, seqlens, cu_q,
                                 (const bf16_t*)q, (bf16_t*)q_out, rope_table, B, total_q, Hq, Hkv, P, max_pages, page_shift, max_pos};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim_256(D, [&](auto d) {
    return paged::for_rope_mode(rope_mode, [&](auto m) { return kva::launch_varlen_bf16<d(), m()>(a, y, s); });
  });
}

CLN_API int cln_kv_append_paged_varlen_d256_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode,
                                                          char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = paged::append_shape_d256(true, B, total_q, Hq, Hkv, max_pages, page, D, rope_mode, rope_mode != 0, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "kv_append_paged_varlen_bf16_rows<D=%d,ROPE=%d> B=%d total_q=%d page=%d: one launch, no workspace; %d x %lld workgroups of 256 "
                         "threads (a packed row x the 16-byte pieces of its %d K, %d V and %d q rows, %d threads per row), the sequence of a row by "
                         "binary search over the device-side offsets, length and table entry through uniform loads, %s%s, plain stores into the "
                         "pools; deterministic",
                         D, rope_mode, B, total_q, page, total_q, y, Hkv, Hkv, rope_mode ? Hq : 0, rope_mode == 1 ? D / 16 : D / 8,
                         paged::kRot[rope_mode], rope_mode ? " in fp32 from the cos/sin table with one rounding at the store, V copied" : "");
  return n < len ? n : len - 1;
}
