// Compile unit of the paged decode attention entries cln_fa2_decode_paged_plan / cln_fa2_decode_paged / cln_fa2_decode_paged_describe
// (include/cln_amd_ext.h; kernels: flash_attn_decode_paged.cuh).
#include "flash_attn_decode_paged.cuh"
#include "paged_entry.h"

namespace {

// paged::decode_plan for one query token per sequence and the key step of this kernel, a function of D that is not asked of a D <= 0
int paged_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  return paged::decode_plan(B, 1, Hq, Hkv, max_pages, page, D, D > 0 ? fa2d::key_step(D) : 0, g, p);
}

}  // namespace

CLN_API int cln_fa2_decode_paged_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk, long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged_plan(B, Hq, Hkv, max_pages, page, D, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens, void* o,
                                 float* lse, void* workspace, long long workspace_bytes, int B, int Hq, int Hkv, int P, int max_pages, int page, int D,
                                 void* stream) {
  const void* in[] = {q, k_pages, v_pages, block_table, seqlens};
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  const int rc = paged::decode_args(in, 5, {o, lse, workspace}, workspace_bytes, P, paged_plan(B, Hq, Hkv, max_pages, page, D, &g, &p), p);
  if (rc != CLN_OK) return rc;
  const fa2d::PagedKV kv = {(const half_t*)k_pages, (const half_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(
      D, [&](auto d) { return fa2d::launch_decode_paged<d()>(g.group, q, kv, seqlens, o, lse, workspace, B, p.splits, p.chunk, s); });
}

CLN_API int cln_fa2_decode_paged_describe(int B, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = paged_plan(B, Hq, Hkv, max_pages, page, D, &g, &p);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "fa2_decode_paged<D=%d,G=%d> S=%d C=%d page=%d: 4 waves stream %d-key steps of K and V rows through the block table to "
                         "registers, each row loaded once for the %d query heads of its KV head, fp32 scores, online softmax",
                         D, g.group, p.splits, p.chunk, page, fa2d::key_step(D), g.group);
  return fa2d::describe_tail(buf, len, n, p, D, "query head", "");
}
