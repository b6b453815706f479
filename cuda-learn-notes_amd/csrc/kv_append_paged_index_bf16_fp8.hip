// Compile unit of the quantising packed append to the paged index-key cache of DeepSeek-V3.2's indexer held in FP8 with per-token scales:
// cln_kv_append_paged_index_bf16_fp8 / cln_kv_append_paged_index_bf16_fp8_describe (include/cln_amd_ext.h; kernel:
// kv_append_paged_index_bf16_fp8.cuh). The checks are kv_append_paged_index_bf16.hip's with one more: -1 for a missing,
// misaligned or aliased pointer, P <= 0, a scale_pow2 that is neither 0 nor 1, or a non-positive dimension; -2 for another page or
// max_pages page >= 2^31.
#include "kv_append_paged_index_bf16_fp8.cuh"
#include "paged_entry.h"

static_assert(kva::kIdx8Dim == paged::kIdxDim && paged::kIdxRowsPerWg * (kva::kIdx8Dim / 8) == kva::kThreads,
              "paged::index_append_shape counts this kernel's rows per workgroup");

CLN_API int cln_kv_append_paged_index_bf16_fp8(const void* k_idx_new, void* idx_pool, const int* block_table, const int* seqlens,
                                               const int* cu_q, int B, int total_q, int P, int max_pages, int page, int scale_pow2,
                                               void* stream) {
  const void* const in[] = {k_idx_new, block_table, seqlens, cu_q};
  const int al16[] = {1, 0, 0, 0};
  int rc = paged::index_args(in, al16, 4, idx_pool, 16);
  if (rc != CLN_OK) return rc;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  if (scale_pow2 != 0 && scale_pow2 != 1) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long wgs = 0;
  rc = paged::index_append_shape(B, total_q, max_pages, page, &page_shift, &wgs);
  if (rc != CLN_OK) return rc;
  const kva::ArgsIndexBf16Fp8 a = {(const bf16_t*)k_idx_new, (uint8_t*)idx_pool, block_table, seqlens, cu_q, B, total_q, P, max_pages, page_shift,
                                   scale_pow2};
  return kva::launch_index_bf16_fp8(a, wgs, (hipStream_t)stream);
}

CLN_API int cln_kv_append_paged_index_bf16_fp8_describe(int B, int total_q, int max_pages, int page, int scale_pow2, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  if (scale_pow2 != 0 && scale_pow2 != 1) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long wgs = 0;
  const int rc = paged::index_append_shape(B, total_q, max_pages, page, &page_shift, &wgs);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "kv_append_paged_index_bf16_fp8_rows B=%d total_q=%d page=%d scale_pow2=%d: one launch, no workspace, no LDS, no atomics; "
                         "%lld workgroups of 256 threads (%d packed rows each x the %d 16-byte pieces of an index key of %d dims: 16 bytes in, 8 "
                         "bytes out a thread), the sequence of a row by binary search over the device-side offsets, packed row cu_q[b] + i "
                         "quantised to cache position seqlens[b] - T_b + i through the block table; a page is %d bytes: codes [%d,%d] e4m3fn at "
                         "byte 128 r, then scales [%d] fp32 at byte %d + 4 r; per token in IEEE fp32 a = max(amax, 1e-4), scale = a / 448%s, inv "
                         "= 1 / scale, code = e4m3fn rne of clamp(k inv, -448, 448); the amax over the 16 lanes of a row by four DPP moves (the "
                         "lanes of a row leave or stay together), lane 0 stores the scale; no rotation; plain stores into the pool; "
                         "deterministic",
                         B, total_q, page, scale_pow2, wgs, paged::kIdxRowsPerWg, paged::kIdxDim / 8, paged::kIdxDim, kva::kIdx8RowBytes * page,
                         page, paged::kIdxDim, page, paged::kIdxDim * page,
                         scale_pow2 ? " rounded up to a power of two on its bits (ue8m0)" : "");
  return n < len ? n : len - 1;
}
