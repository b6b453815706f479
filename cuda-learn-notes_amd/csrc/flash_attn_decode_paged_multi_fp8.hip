// Compile unit of the FP8 multi-token paged decode attention entries cln_fa2_decode_paged_multi_fp8_plan / cln_fa2_decode_paged_multi_fp8 /
// cln_fa2_decode_paged_multi_fp8_describe (include/cln_amd_ext.h; kernels: flash_attn_decode_paged_multi_fp8.cuh). The split plan is
// paged::multi_plan (paged_entry.h): the key step is that of the fp16 kernel, so the two entries plan alike.
#include "flash_attn_decode_paged_multi_fp8.cuh"
#include "paged_entry.h"

CLN_API int cln_fa2_decode_paged_multi_fp8_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk,
                                                long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged::multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                           const float* k_scale, const float* v_scale, void* o, float* lse, void* workspace,
                                           long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages, int page, int D,
                                           void* stream) {
  const void* in[] = {q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale};  // the last four: 4-byte aligned
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  const int rc = paged::decode_args(in, 7, {o, lse, workspace}, workspace_bytes, P, paged::multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p), p);
  if (rc != CLN_OK) return rc;
  const fa2d::PagedKV8 kv = {(const uint8_t*)k_pages, (const uint8_t*)v_pages, k_scale, v_scale, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(D, [&](auto d) {
    return paged::for_row_tiles(paged::multi_tiles(T, g), [&](auto mt) {
      return fa2pm::launch_decode_paged_multi_fp8<d(), mt()>(q, kv, seqlens, o, lse, workspace, B, T, g.g_shift, p.splits, p.chunk, s);
    });
  });
}

CLN_API int cln_fa2_decode_paged_multi_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = paged::multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p);
  if (rc != CLN_OK) return rc;
  const int tiles = paged::multi_tiles(T, g);
  const int n = snprintf(buf, len,
                         "fa2_decode_paged_multi_fp8<D=%d,MT=%d> T=%d G=%d S=%d C=%d page=%d: 4 waves split the %d-key steps, e4m3 K and V rows "
                         "through the block table to registers, 16 bytes per lane, converted to fp16 once (v_cvt_scalef32_pk_f16_fp8, exact): K "
                         "to MFMA fragments, V through a transposed LDS read, each row loaded once for the %d query rows (T x G, %d tiles of 16) "
                         "of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16, fp32 scores times k_scale, causal mask by "
                         "select, online softmax, the partial times v_scale",
                         D, tiles, T, g.group, p.splits, p.chunk, page, fa2pm::kKeyStep, T * g.group, tiles);
  return fa2d::describe_tail(buf, len, n, p, D, "query row", "");
}
