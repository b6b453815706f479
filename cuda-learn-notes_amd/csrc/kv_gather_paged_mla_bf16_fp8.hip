// Compile unit of the packed gather out of a paged latent cache held in FP8 into bf16 rows (multi-head latent attention):
// cln_kv_gather_paged_mla_bf16_fp8 / cln_kv_gather_paged_mla_bf16_fp8_describe (include/cln_amd_ext.h; kernel: kv_gather_paged_mla_bf16_fp8.cuh;
// DESIGN 4.4.19). The checks are paged::mla_gather_args with kv_scale (fp32 [1] on the device, behind cu_k) required, then paged::mla_gather_shape: -1 for a
// missing, misaligned or aliased pointer (starts may be null) or a non-positive dimension; -2 for another page, max_pages page >= 2^31 or a grid
// that does not fit.
#include "kv_gather_paged_mla_bf16_fp8.cuh"
#include "paged_entry.h"

CLN_API int cln_kv_gather_paged_mla_bf16_fp8(const void* pool, const int* block_table, const int* starts, const int* cu_k, const float* kv_scale,
                                             void* out, int B, int total_k, int P, int max_pages, int page, void* stream) {
  int rc = paged::mla_gather_args(pool, block_table, starts, cu_k, kv_scale, true, out, P);
  if (rc != CLN_OK) return rc;
  int page_shift = 0;
  long long y = 0;
  rc = paged::mla_gather_shape(B, total_k, max_pages, page, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const kva::ArgsMlaGatherBf16Fp8 a = {(const uint8_t*)pool, block_table, starts, cu_k, kv_scale, (bf16_t*)out, B, total_k, P, max_pages, page_shift};
  return kva::launch_mla_gather_bf16_fp8(a, y, (hipStream_t)stream);
}

CLN_API int cln_kv_gather_paged_mla_bf16_fp8_describe(int B, int total_k, int max_pages, int page, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = paged::mla_gather_shape(B, total_k, max_pages, page, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "kv_gather_paged_mla_bf16_fp8_rows B=%d total_k=%d page=%d: one launch, no workspace; %d x %lld workgroups of 256 threads (a "
                         "packed row x the %d 8-byte pieces of its latent row [c %d | k_pe %d] of e4m3fn codes), the sequence of a row by binary "
                         "search over the device-side offsets, start and table entry through uniform loads, packed row cu_k[b] + i = cache row "
                         "starts[b] + i as bf16: the code converted (v_cvt_scalef32_pk_bf16_fp8, exact) times kv_scale (fp32 [1] on the device) in "
                         "fp32, rounded once, a cache row at or past max_pages page = %lld written as zeros without a table read; deterministic",
                         B, total_k, page, total_k, y, paged::kMlaDk / 8, paged::kMlaDc, paged::kMlaDr, (long long)max_pages * page);
  return n < len ? n : len - 1;
}
