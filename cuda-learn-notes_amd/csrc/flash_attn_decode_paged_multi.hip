// Compile unit of the multi-token paged decode attention entries cln_fa2_decode_paged_multi_plan / cln_fa2_decode_paged_multi /
// cln_fa2_decode_paged_multi_describe (include/cln_amd_ext.h; kernels: flash_attn_decode_paged_multi.cuh).
#include "flash_attn_decode_paged_multi.cuh"
#include "paged_entry.h"

CLN_API int cln_fa2_decode_paged_multi_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk,
                                            long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged::multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens, void* o,
                                       float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages,
                                       int page, int D, void* stream) {
  const void* in[] = {q, k_pages, v_pages, block_table, seqlens};
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  const int rc = paged::decode_args(in, 5, {o, lse, workspace}, workspace_bytes, P, paged::multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p), p);
  if (rc != CLN_OK) return rc;
  const fa2d::PagedKV kv = {(const half_t*)k_pages, (const half_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(D, [&](auto d) {
    return paged::for_row_tiles(paged::multi_tiles(T, g), [&](auto mt) {
      return fa2pm::launch_decode_paged_multi<d(), mt()>(q, kv, seqlens, o, lse, workspace, B, T, g.g_shift, p.splits, p.chunk, s);
    });
  });
}

CLN_API int cln_fa2_decode_paged_multi_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = paged::multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p);
  if (rc != CLN_OK) return rc;
  const int tiles = paged::multi_tiles(T, g);
  const int n = snprintf(buf, len,
                         "fa2_decode_paged_multi<D=%d,MT=%d> T=%d G=%d S=%d C=%d page=%d: 4 waves split the %d-key steps, K rows through the block "
                         "table straight to MFMA fragments, V rows through a transposed LDS read, each row loaded once for the %d query rows (T x G, "
                         "%d tiles of 16) of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16, fp32 scores, causal mask by "
                         "select, online softmax",
                         D, tiles, T, g.group, p.splits, p.chunk, page, fa2pm::kKeyStep, T * g.group, tiles);
  return fa2d::describe_tail(buf, len, n, p, D, "query row", "");
}
