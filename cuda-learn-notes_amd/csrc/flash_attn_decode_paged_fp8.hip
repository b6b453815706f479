// Compile unit of the FP8 paged decode attention entries cln_fa2_decode_paged_fp8_plan / cln_fa2_decode_paged_fp8 /
// cln_fa2_decode_paged_fp8_describe (include/cln_amd_ext.h; kernels: flash_attn_decode_paged_fp8.cuh).
#include "flash_attn_decode_paged_fp8.cuh"
#include "paged_entry.h"

namespace {

// paged::decode_plan for one query token per sequence and the key step of this kernel, a function of D that is not asked of a D <= 0
int fp8_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  return paged::decode_plan(B, 1, Hq, Hkv, max_pages, page, D, D > 0 ? fa2d::key_step_fp8(D) : 0, g, p);
}

}  // namespace

CLN_API int cln_fa2_decode_paged_fp8_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk,
                                          long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(fp8_plan(B, Hq, Hkv, max_pages, page, D, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                     const float* k_scale, const float* v_scale, void* o, float* lse, void* workspace, long long workspace_bytes,
                                     int B, int Hq, int Hkv, int P, int max_pages, int page, int D, void* stream) {
  const void* in[] = {q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale};  // the last four: 4-byte aligned
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  const int rc = paged::decode_args(in, 7, {o, lse, workspace}, workspace_bytes, P, fp8_plan(B, Hq, Hkv, max_pages, page, D, &g, &p), p);
  if (rc != CLN_OK) return rc;
  const fa2d::PagedKV8 kv = {(const uint8_t*)k_pages, (const uint8_t*)v_pages, k_scale, v_scale, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(
      D, [&](auto d) { return fa2d::launch_decode_paged_fp8<d()>(g.group, q, kv, seqlens, o, lse, workspace, B, p.splits, p.chunk, s); });
}

CLN_API int cln_fa2_decode_paged_fp8_describe(int B, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = fp8_plan(B, Hq, Hkv, max_pages, page, D, &g, &p);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "fa2_decode_paged_fp8<D=%d,G=%d> S=%d C=%d page=%d: 4 waves stream %d-key steps of e4m3 K and V rows through the block "
                         "table to registers, 8 bytes per lane and row, each row loaded and converted to fp32 once for the %d query heads of its "
                         "KV head, fp32 scores times k_scale, online softmax, the partial times v_scale",
                         D, g.group, p.splits, p.chunk, page, fa2d::key_step_fp8(D), g.group);
  return fa2d::describe_tail(buf, len, n, p, D, "query head", "");
}
