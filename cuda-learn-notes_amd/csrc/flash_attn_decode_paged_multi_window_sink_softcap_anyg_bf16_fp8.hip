// Compile unit of the sliding-window multi-token paged decode attention entries with attention sinks, bf16 queries and FP8 pools, any group size
// G = Hq / Hkv in 1 ... 16, a softmax scale of the caller's and optional logit soft-capping:
// cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan / cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8 /
// cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_describe (include/cln_amd_ext.h; kernel:
// flash_attn_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8.cuh): the any-G FP8 entry with the two floats behind `window`, checked first;
// the plan takes neither float and is the any-G entry's. softcap == 0 launches the CAP = false instantiations. The checks, their order and the
// text are paged::window_decode / softcap_describe_then / window_decode_describe (paged_entry.h).
#include "flash_attn_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8.cuh"
#include "paged_entry.h"

static_assert(fa2b::kMultiKeyStep == fa2pm::kKeyStep, "paged::multi_window_plan_anyg plans with the key step of this kernel");

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D,
                                                                              int window, int* splits, int* chunk, long long* workspace_bytes) {
  return paged::window_plan_entry<paged::kAnyG>({B, T, Hq, Hkv, max_pages, page, D, window}, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8(const void* q, const void* k_pages, const void* v_pages,
                                                                         const int* block_table, const int* seqlens, const float* k_scale,
                                                                         const float* v_scale, const float* sinks, void* o, float* lse,
                                                                         void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv,
                                                                         int P, int max_pages, int page, int D, int window, float softmax_scale,
                                                                         float softcap, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, sinks};
  const hipStream_t s = (hipStream_t)stream;
  return paged::window_decode<fa2d::PagedKV8, paged::kAnyG>(
      in, sinks ? 8 : 7, o, lse, workspace, workspace_bytes, P, {B, T, Hq, Hkv, max_pages, page, D, window, softmax_scale, softcap},
      [&](auto d, auto mt, auto cap, const fa2d::PagedKV8& kv, const paged::WindowLaunch& w) {
        return fa2b::launch_decode_paged_multi_window_sink_softcap_anyg_fp8<d(), mt(), cap()>(
            q, kv, seqlens, sinks, o, lse, workspace, B, T, w.g.group, w.p.splits, w.p.chunk, window, w.sc.mult, w.sc.pre, w.sc.cap2, s);
      });
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D,
                                                                                  int window, float softmax_scale, float softcap, char* buf,
                                                                                  int len) {
  const paged::WindowArgs a = {B, T, Hq, Hkv, max_pages, page, D, window, softmax_scale, softcap};
  return paged::softcap_describe_then(buf, len, "fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_mfma", a, true, [&](char* rest, int n) {
    return paged::window_decode_describe<fa2d::PagedKV8, paged::kAnyG>("fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_mfma",
                                                                       paged::kSinksOptional, a, rest, n);
  });
}
