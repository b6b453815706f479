// Compile unit of the paged decode attention entries cln_fa2_decode_paged_plan / cln_fa2_decode_paged / cln_fa2_decode_paged_describe
// (include/cln_amd_ext.h; kernels: flash_attn_decode_paged.cuh).
#include "flash_attn_decode_paged.cuh"

namespace {

// The split plan (fa2d::split_plan): a function of (B, Hq, Hkv, max_pages, page, D) only. A workgroup serves a whole group of query heads, so the
// workgroup count is B Hkv S.
int paged_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  if (B <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  const int step = fa2d::key_step(D);
  return fa2d::split_plan((long long)B * Hkv, (long long)B * Hq, g->Nmax, page > step ? page : step, D, p);
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
  int rc = fa2d::check_pointers(in, 5, 3, {o, lse, workspace});
  if (rc != CLN_OK) return rc;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  rc = paged_plan(B, Hq, Hkv, max_pages, page, D, &g, &p);
  if (rc != CLN_OK) return rc;
  if (!fa2d::workspace_fits(p, workspace, workspace_bytes)) return CLN_ERR_BAD_ARG;
  const fa2d::PagedKV kv = {(const half_t*)k_pages, (const half_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  if (D == 64) return fa2d::launch_decode_paged<64>(g.group, q, kv, seqlens, o, lse, workspace, B, p.splits, p.chunk, s);
  return fa2d::launch_decode_paged<128>(g.group, q, kv, seqlens, o, lse, workspace, B, p.splits, p.chunk, s);
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
