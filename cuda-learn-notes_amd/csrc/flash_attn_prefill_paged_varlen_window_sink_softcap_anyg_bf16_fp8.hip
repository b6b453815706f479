// Compile unit of the sliding-window packed paged prefill attention entries with attention sinks, bf16 queries and FP8 pools, any group size
// G = Hq / Hkv in 1 ... 16, a softmax scale of the caller's and optional logit soft-capping:
// cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8 / cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8_describe
// (include/cln_amd_ext.h; kernel: flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8.cuh): the any-G FP8 entry with the two floats
// behind `window`, checked first; softcap == 0 launches the CAP = false instantiation. The checks, their order and the text are
// paged::window_prefill / softcap_describe_then / window_prefill_describe (paged_entry.h).
#include "flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8.cuh"
#include "paged_entry.h"

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8(const void* q, const void* k_pages, const void* v_pages,
                                                                           const int* block_table, const int* seqlens, const int* cu_q,
                                                                           const float* k_scale, const float* v_scale, const float* sinks, void* o,
                                                                           float* lse, int B, int total_q, int Hq, int Hkv, int P, int max_pages,
                                                                           int page, int D, int window, float softmax_scale, float softcap,
                                                                           void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, sinks};
  const hipStream_t s = (hipStream_t)stream;
  return paged::window_prefill<fa2d::PagedKV8, paged::kAnyG>(
      in, sinks ? 9 : 8, o, lse, P, {B, total_q, Hq, Hkv, max_pages, page, D, window, softmax_scale, softcap},
      [&](auto d, auto cap, const fa2d::PagedKV8& kv, const paged::WindowLaunch& w) {
        return fa2b::launch_prefill_paged_varlen_window_sink_softcap_anyg_fp8<d(), cap()>(q, kv, seqlens, cu_q, sinks, o, lse, B, total_q, w.g.group,
                                                                                          w.slots, window, w.sc.mult, w.sc.pre, w.sc.cap2, s);
      });
}

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page,
                                                                                    int D, int window, float softmax_scale, float softcap,
                                                                                    char* buf, int len) {
  const paged::WindowArgs a = {B, total_q, Hq, Hkv, max_pages, page, D, window, softmax_scale, softcap};
  return paged::softcap_describe_then(buf, len, "fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8_mfma", a, true, [&](char* rest, int n) {
    return paged::window_prefill_describe<fa2d::PagedKV8, paged::kAnyG>("fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8_mfma",
                                                                        paged::kSinksOptional, a, rest, n);
  });
}
