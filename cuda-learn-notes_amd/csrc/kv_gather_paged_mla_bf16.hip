// Compile unit of the bf16 packed gather out of a paged latent cache (multi-head latent attention): cln_kv_gather_paged_mla_bf16 /
// cln_kv_gather_paged_mla_bf16_describe (include/cln_amd_ext.h; kernel: kv_gather_paged_mla_bf16.cuh). The checks are
// paged::mla_gather_args, then paged::mla_gather_shape: -1 for a missing, misaligned or aliased pointer (starts may be null) or a non-positive dimension; -2 for
// another page, max_pages page >= 2^31 or a grid that does not fit.
#include "kv_gather_paged_mla_bf16.cuh"
#include "paged_entry.h"

CLN_API int cln_kv_gather_paged_mla_bf16(const void* pool, const int* block_table, const int* starts, const int* cu_k, void* out, int B,
                                         int total_k, int P, int max_pages, int page, void* stream) {
  int rc = paged::mla_gather_args(pool, block_table, starts, cu_k, nullptr, false, out, P);
  if (rc != CLN_OK) return rc;
  int page_shift = 0;
  long long y = 0;
  rc = paged::mla_gather_shape(B, total_k, max_pages, page, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const kva::ArgsMlaGatherBf16 a = {(const bf16_t*)pool, block_table, starts, cu_k, (bf16_t*)out, B, total_k, P, max_pages, page_shift};
  return kva::launch_mla_gather_bf16(a, y, (hipStream_t)stream);
}

CLN_API int cln_kv_gather_paged_mla_bf16_describe(int B, int total_k, int max_pages, int page, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = paged::mla_gather_shape(B, total_k, max_pages, page, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "kv_gather_paged_mla_bf16_rows B=%d total_k=%d page=%d: one launch, no workspace; %d x %lld workgroups of 256 threads (a "
                         "packed row x the %d 16-byte pieces of its latent row [c %d | k_pe %d]), the sequence of a row by binary search over the "
                         "device-side offsets, start and table entry through uniform loads, packed row cu_k[b] + i = cache row starts[b] + i bit for "
                         "bit, a cache row at or past max_pages page = %lld written as zeros without a table read; deterministic",
                         B, total_k, page, total_k, y, paged::kMlaDk / 8, paged::kMlaDc, paged::kMlaDr, (long long)max_pages * page);
  return n < len ? n : len - 1;
}
