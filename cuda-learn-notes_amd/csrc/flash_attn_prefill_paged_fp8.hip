// Compile unit of the FP8 paged prefill attention entries cln_fa2_prefill_paged_fp8 / cln_fa2_prefill_paged_fp8_describe
// (include/cln_amd_ext.h; kernel: flash_attn_prefill_paged_fp8.cuh).
#include "flash_attn_prefill_paged_fp8.cuh"
#include "paged_entry.h"

CLN_API int cln_fa2_prefill_paged_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                      const float* k_scale, const float* v_scale, void* o, float* lse, int B, int T, int Hq, int Hkv, int P,
                                      int max_pages, int page, int D, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale};  // 16-byte aligned up to the table, 4-byte from there on
  int rc = paged::prefill_args(in, 7, o, lse, P);
  if (rc != CLN_OK) return rc;
  fa2d::PagedGeometry g;
  long long tiles = 0;
  rc = paged::prefill_shape(B, T, Hq, Hkv, max_pages, page, D, &g, &tiles);
  if (rc != CLN_OK) return rc;
  const fa2d::PagedKV8 kv = {(const uint8_t*)k_pages, (const uint8_t*)v_pages, k_scale, v_scale, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(D, [&](auto d) { return fa2pp::launch_prefill_paged_fp8<d()>(q, kv, seqlens, o, lse, B, T, g.g_shift, tiles, s); });
}

CLN_API int cln_fa2_prefill_paged_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  long long tiles = 0;
  const int rc = paged::prefill_shape(B, T, Hq, Hkv, max_pages, page, D, &g, &tiles);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "fa2_prefill_paged_fp8<D=%d,G=%d> T=%d page=%d rows=%d keys=%d: one launch, no workspace; %lld workgroups of 256 threads "
                         "(%lld (sequence, KV head) pairs x %lld tiles of %d of the %lld query rows t G + g, 32 rows per wave), each walks the keys "
                         "below the causal edge of its last token in steps of %d, e4m3 K and V rows through the block table, 8 bytes per thread "
                         "and row, converted to fp16 once on their way to LDS (v_cvt_scalef32_pk_f16_fp8, exact), S^T = K Q^T and O^T = V^T P^T on "
                         "v_mfma_f32_16x16x32_f16, V through ds_read_b64_tr_b16, fp32 scores times k_scale, causal mask by select on the steps that "
                         "cross the edge, online softmax, the normalisation times v_scale, no split over the keys; deterministic",
                         D, g.group, T, page, fa2pp::kRowTile, fa2pp::kKeyStep, (long long)B * Hkv * tiles, (long long)B * Hkv, tiles,
                         fa2pp::kRowTile, (long long)T * g.group, fa2pp::kKeyStep);
  return n < len ? n : len - 1;
}
