// Compile unit of the bf16 packed append to the paged index-key cache of DeepSeek-V3.2's indexer: cln_kv_append_paged_index_bf16 /
// cln_kv_append_paged_index_bf16_describe (include/cln_amd_ext.h; kernel: kv_append_paged_index_bf16.cuh). The checks follow
// kv_append_paged_mla_bf16.hip: -1 for a missing, misaligned or aliased pointer, P <= 0 or a non-positive dimension; -2 for another page or
// max_pages page >= 2^31.
#include "kv_append_paged_index_bf16.cuh"
#include "paged_entry.h"

static_assert(kva::kIdxDim == paged::kIdxDim && paged::kIdxRowsPerWg * (kva::kIdxDim / 8) == kva::kThreads,
              "paged::index_append_shape counts this kernel's rows per workgroup");

CLN_API int cln_kv_append_paged_index_bf16(const void* k_idx_new, void* idx_pool, const int* block_table, const int* seqlens, const int* cu_q,
                                           int B, int total_q, int P, int max_pages, int page, void* stream) {
  const void* const in[] = {k_idx_new, block_table, seqlens, cu_q};
  const int al16[] = {1, 0, 0, 0};
  int rc = paged::index_args(in, al16, 4, idx_pool, 16);
  if (rc != CLN_OK) return rc;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long wgs = 0;
  rc = paged::index_append_shape(B, total_q, max_pages, page, &page_shift, &wgs);
  if (rc != CLN_OK) return rc;
  const kva::ArgsIndexBf16 a = {(const bf16_t*)k_idx_new, (bf16_t*)idx_pool, block_table, seqlens, cu_q, B, total_q, P, max_pages, page_shift};
  return kva::launch_index_bf16(a, wgs, (hipStream_t)stream);
}

CLN_API int cln_kv_append_paged_index_bf16_describe(int B, int total_q, int max_pages, int page, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long wgs = 0;
  const int rc = paged::index_append_shape(B, total_q, max_pages, page, &page_shift, &wgs);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "kv_append_paged_index_bf16_rows B=%d total_q=%d page=%d: one launch, no workspace; %lld workgroups of 256 threads (%d "
                         "packed rows each x the %d 16-byte pieces of an index key of %d dims), the sequence of a row by binary search over the "
                         "device-side offsets, packed row cu_q[b] + i copied bit for bit to cache position seqlens[b] - T_b + i through the block "
                         "table, no rotation (the model rotates, then applies a Hadamard transform, before it caches the key), plain stores into "
                         "the pool; deterministic",
                         B, total_q, page, wgs, paged::kIdxRowsPerWg, paged::kIdxDim / 8, paged::kIdxDim);
  return n < len ? n : len - 1;
}
