// Compile unit of the bf16 sliding-window multi-token paged decode attention entries with attention sinks for any group size G = Hq / Hkv in
// 1 ... 16: cln_fa2_decode_paged_multi_window_sink_anyg_bf16_plan / cln_fa2_decode_paged_multi_window_sink_anyg_bf16 /
// cln_fa2_decode_paged_multi_window_sink_anyg_bf16_describe (include/cln_amd_ext.h; kernel: flash_attn_decode_paged_multi_window_sink_anyg_bf16.cuh):
// bf16 pools, any G with T <= 8 and T G <= 64 (paged::multi_window_plan_anyg: the power-of-two siblings' fa2d::split_plan of the same numbers);
// sinks, last of the inputs, may be null (no sink) and is checked like the others when it is not. The plan, the checks, their order and the text
// are paged::window_plan_entry / window_decode / window_decode_describe (paged_entry.h).
#include "flash_attn_decode_paged_multi_window_sink_anyg_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2b::kMultiKeyStep == fa2pm::kKeyStep, "paged::multi_window_plan_anyg plans with the key step of this kernel");

CLN_API int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                  int* splits, int* chunk, long long* workspace_bytes) {
  return paged::window_plan_entry<paged::kAnyG>({B, T, Hq, Hkv, max_pages, page, D, window}, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_anyg_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                             const int* seqlens, const float* sinks, void* o, float* lse, void* workspace,
                                                             long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages,
                                                             int page, int D, int window, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, sinks};
  const hipStream_t s = (hipStream_t)stream;
  return paged::window_decode<fa2b::PagedKV, paged::kAnyG>(
      in, sinks ? 6 : 5, o, lse, workspace, workspace_bytes, P, {B, T, Hq, Hkv, max_pages, page, D, window},
      [&](auto d, auto mt, auto, const fa2b::PagedKV& kv, const paged::WindowLaunch& w) {
        return fa2b::launch_decode_paged_multi_window_sink_anyg<d(), mt()>(q, kv, seqlens, sinks, o, lse, workspace, B, T, w.g.group, w.p.splits,
                                                                           w.p.chunk, window, s);
      });
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                      char* buf, int len) {
  return paged::window_decode_describe<fa2b::PagedKV, paged::kAnyG>("fa2_decode_paged_multi_window_sink_anyg_bf16_mfma", paged::kSinksOptional,
                                                                    {B, T, Hq, Hkv, max_pages, page, D, window}, buf, len);
}
