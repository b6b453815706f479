// Compile unit of the bf16 sliding-window packed paged prefill attention entries with attention sinks, any group size G = Hq / Hkv in 1 ... 16, a
// softmax scale of the caller's and optional logit soft-capping: cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16 /
// cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_describe (include/cln_amd_ext.h; kernel:
// flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_bf16.cuh). The two floats stand behind `window` and are checked first, before any
// pointer is looked at (paged::softcap_arg); every other check and status code is that of flash_attn_prefill_paged_varlen_window_sink_anyg_bf16.hip,
// argument by argument. softcap == 0 launches the CAP = false instantiation.
#include "flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_bf16.cuh"
#include "paged_entry.h"

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D,
                                                                        int window, char* buf, int len);

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16(const void* q, const void* k_pages, const void* v_pages,
                                                                       const int* block_table, const int* seqlens, const int* cu_q,
                                                                       const float* sinks, void* o, float* lse, int B, int total_q, int Hq, int Hkv,
                                                                       int P, int max_pages, int page, int D, int window, float softmax_scale,
                                                                       float softcap, void* stream) {
  paged::SoftCap sc;
  int rc = paged::softcap_arg(softmax_scale, softcap, D, &sc);
  if (rc != CLN_OK) return rc;
  // 16-byte aligned up to the table, 4-byte from there on; sinks counts only when given
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, cu_q, sinks};
  rc = paged::prefill_args(in, sinks ? 7 : 6, o, lse, P);
  if (rc != CLN_OK) return rc;
  fa2d::PagedGeometry g;
  long long slots = 0;
  rc = paged::prefill_varlen_shape_anyg(B, total_q, Hq, Hkv, max_pages, page, D, &g, &slots);
  if (rc == CLN_OK) rc = paged::window_arg(window);
  if (rc != CLN_OK) return rc;
  const fa2b::PagedKV kv = {(const bf16_t*)k_pages, (const bf16_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(D, [&](auto d) {
    if (sc.cap)
      return fa2b::launch_prefill_paged_varlen_window_sink_softcap_anyg<d(), true>(q, kv, seqlens, cu_q, sinks, o, lse, B, total_q, g.group, slots,
                                                                                   window, sc.mult, sc.pre, sc.cap2, s);
    return fa2b::launch_prefill_paged_varlen_window_sink_softcap_anyg<d(), false>(q, kv, seqlens, cu_q, sinks, o, lse, B, total_q, g.group, slots,
                                                                                  window, sc.mult, 0.0f, 0.0f, s);
  });
}

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D,
                                                                                int window, float softmax_scale, float softcap, char* buf,
                                                                                int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  paged::SoftCap sc;
  int rc = paged::softcap_arg(softmax_scale, softcap, D, &sc);
  if (rc != CLN_OK) return rc;
  const int n = paged::softcap_describe(buf, len, "fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_mfma", D, softmax_scale, softcap, sc, false);
  rc = cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_describe(B, total_q, Hq, Hkv, max_pages, page, D, window, buf + n, len - n);
  return rc < 0 ? rc : n + rc;
}
