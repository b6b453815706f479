// Compile unit of the bf16 sliding-window multi-token paged decode attention entries with attention sinks, any group size G = Hq / Hkv in 1 ... 16,
// a softmax scale of the caller's and optional logit soft-capping: cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan /
// cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16 / cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_describe
// (include/cln_amd_ext.h; kernel: flash_attn_decode_paged_multi_window_sink_softcap_anyg_bf16.cuh). The plan takes neither float and is
// paged::multi_window_plan_anyg unchanged: the splits, the chunk and the workspace of the any-G entry for the same numbers. The two floats stand
// behind `window` and are checked first, before any pointer is looked at (paged::softcap_arg); every other check and status code is that of
// flash_attn_decode_paged_multi_window_sink_anyg_bf16.hip, argument by argument. softcap == 0 launches the CAP = false instantiations.
#include "flash_attn_decode_paged_multi_window_sink_softcap_anyg_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2b::kMultiKeyStep == fa2pm::kKeyStep, "paged::multi_window_plan_anyg plans with the key step of this kernel");
static_assert(paged::kMaxRowsAnyG == 4 * 16, "paged::for_row_tiles has 1 ... 4 row tiles of 16");

CLN_API int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                      char* buf, int len);

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                          int* splits, int* chunk, long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged::multi_window_plan_anyg(B, T, Hq, Hkv, max_pages, page, D, window, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                                     const int* seqlens, const float* sinks, void* o, float* lse, void* workspace,
                                                                     long long workspace_bytes, int B, int T, int Hq, int Hkv, int P,
                                                                     int max_pages, int page, int D, int window, float softmax_scale,
                                                                     float softcap, void* stream) {
  paged::SoftCap sc;
  int rc = paged::softcap_arg(softmax_scale, softcap, D, &sc);
  if (rc != CLN_OK) return rc;
  const void* in[] = {q, k_pages, v_pages, block_table, seqlens, sinks};  // the last three: 4-byte aligned; sinks only when given
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  rc = paged::decode_args(in, sinks ? 6 : 5, {o, lse, workspace}, workspace_bytes, P,
                          paged::multi_window_plan_anyg(B, T, Hq, Hkv, max_pages, page, D, window, &g, &p), p);
  if (rc != CLN_OK) return rc;
  const fa2b::PagedKV kv = {(const bf16_t*)k_pages, (const bf16_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(D, [&](auto d) {
    return paged::for_row_tiles(paged::multi_tiles(T, g), [&](auto mt) {
      if (sc.cap)
        return fa2b::launch_decode_paged_multi_window_sink_softcap_anyg<d(), mt(), true>(q, kv, seqlens, sinks, o, lse, workspace, B, T, g.group,
                                                                                         p.splits, p.chunk, window, sc.mult, sc.pre, sc.cap2, s);
      return fa2b::launch_decode_paged_multi_window_sink_softcap_anyg<d(), mt(), false>(q, kv, seqlens, sinks, o, lse, workspace, B, T, g.group,
                                                                                        p.splits, p.chunk, window, sc.mult, 0.0f, 0.0f, s);
    });
  });
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D,
                                                                              int window, float softmax_scale, float softcap, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  paged::SoftCap sc;
  int rc = paged::softcap_arg(softmax_scale, softcap, D, &sc);
  if (rc != CLN_OK) return rc;
  const int n = paged::softcap_describe(buf, len, "fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_mfma", D, softmax_scale, softcap, sc, false);
  rc = cln_fa2_decode_paged_multi_window_sink_anyg_bf16_describe(B, T, Hq, Hkv, max_pages, page, D, window, buf + n, len - n);
  return rc < 0 ? rc : n + rc;
}
