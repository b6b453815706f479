// Compile unit of the packed variable-length paged KV-cache append entries from bf16 rows into FP8 pools cln_kv_append_paged_varlen_bf16_fp8 /
// cln_kv_append_paged_varlen_bf16_fp8_describe (include/cln_amd_ext.h; kernel: kv_append_paged_varlen_bf16_fp8.cuh). The checks and the status codes
// are those of kv_append_paged_varlen_bf16.hip; k_scale and v_scale are two more required inputs behind cu_q, 4-byte aligned, as
// kv_append_paged_fp8.hip has them behind seqlens.
#include "kv_append_paged_varlen_bf16_fp8.cuh"
#include "paged_entry.h"

CLN_API int cln_kv_append_paged_varlen_bf16_fp8(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table,
                                                const int* seqlens, const int* cu_q, const float* k_scale, const float* v_scale, const void* q,
                                                void* q_out, const float* rope_table, int B, int total_q, int Hq, int Hkv, int P, int max_pages,
                                                int page, int D, int max_pos, int rope_mode, void* stream) {
  const void* const in[] = {k_new, v_new, block_table, seqlens, cu_q, k_scale, v_scale, q, rope_table};  // the required inputs, then q and rope_table
  const int al4[] = {0, 0, 1, 1, 1, 1, 1, 0, 1};
  int rc = paged::append_args(in, al4, 7, {k_pages, v_pages, q_out}, P, max_pos, rope_mode);
  if (rc != CLN_OK) return rc;
  int page_shift = 0;
  long long y = 0;
  rc = paged::append_shape(true, B, total_q, Hq, Hkv, max_pages, page, D, rope_mode, q != nullptr, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const kva::ArgsVarlenBf16Fp8 a = {(const bf16_t*)k_new, (const bf16_t*)v_new, (uint8_t*)k_pages, (uint8_t*)v_pages, block_table, seqlens, cu_q,
                                    k_scale, v_scale, (const bf16_t*)q, (bf16_t*)q_out, rope_table, B, total_q, Hq, Hkv, P, max_pages, page_shift,
                                    max_pos};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(D, [&](auto d) {
    return paged::for_rope_mode(rope_mode, [&](auto m) { return kva::launch_varlen_bf16_fp8<d(), m()>(a, y, s); });
  });
}

CLN_API int cln_kv_append_paged_varlen_bf16_fp8_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode,
                                                         char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = paged::append_shape(true, B, total_q, Hq, Hkv, max_pages, page, D, rope_mode, rope_mode != 0, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "kv_append_paged_varlen_bf16_fp8_rows<D=%d,ROPE=%d> B=%d total_q=%d page=%d: one launch, no workspace; %d x %lld workgroups "
                         "of 256 threads (a packed row x the 8-element pieces of its %d K, %d V and %d q rows), the sequence of a row by binary "
                         "search over the device-side offsets, length and table entry through uniform loads, %s%s, K and V times 1 / scale of "
                         "their KV head in fp32, clamped to +-448 and rounded to nearest even to e4m3, 8-byte plain stores into the pools; "
                         "deterministic",
                         D, rope_mode, B, total_q, page, total_q, y, Hkv, Hkv, rope_mode ? Hq : 0,
                         rope_mode ? paged::kRot[rope_mode] : "rows not rotated",
                         rope_mode ? " in fp32 from the cos/sin table, q rounded once to bf16 at the store" : "");
  return n < len ? n : len - 1;
}
