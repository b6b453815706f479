// Compile unit of the sliding-window multi-token paged decode attention entries with attention sinks, bf16 queries and FP8 pools
// cln_fa2_decode_paged_multi_window_sink_bf16_fp8_plan / cln_fa2_decode_paged_multi_window_sink_bf16_fp8 /
// cln_fa2_decode_paged_multi_window_sink_bf16_fp8_describe (include/cln_amd_ext.h; kernel: flash_attn_decode_paged_multi_window_sink_bf16_fp8.cuh):
// FP8 pools, G a power of two; k_scale and v_scale are two more required inputs behind seqlens, where flash_attn_decode_paged_multi_fp8.hip has
// them; sinks, last, may be null (no sink) and is checked like the others when it is not. Neither the pools' element size nor the sink changes the
// splits or the workspace. The plan, the checks, their order and the text are paged::window_plan_entry / window_decode / window_decode_describe
// (paged_entry.h).
#include "flash_attn_decode_paged_multi_window_sink_bf16_fp8.cuh"
#include "paged_entry.h"

static_assert(fa2b::kMultiKeyStep == fa2pm::kKeyStep, "paged::multi_window_plan plans with the key step of this kernel");

CLN_API int cln_fa2_decode_paged_multi_window_sink_bf16_fp8_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                 int* splits, int* chunk, long long* workspace_bytes) {
  return paged::window_plan_entry<paged::kPow2G>({B, T, Hq, Hkv, max_pages, page, D, window}, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_bf16_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                            const int* seqlens, const float* k_scale, const float* v_scale, const float* sinks,
                                                            void* o, float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq,
                                                            int Hkv, int P, int max_pages, int page, int D, int window, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, sinks};
  const hipStream_t s = (hipStream_t)stream;
  return paged::window_decode<fa2d::PagedKV8, paged::kPow2G>(
      in, sinks ? 8 : 7, o, lse, workspace, workspace_bytes, P, {B, T, Hq, Hkv, max_pages, page, D, window},
      [&](auto d, auto mt, auto, const fa2d::PagedKV8& kv, const paged::WindowLaunch& w) {
        return fa2b::launch_decode_paged_multi_window_sink_fp8<d(), mt()>(q, kv, seqlens, sinks, o, lse, workspace, B, T, w.g.g_shift, w.p.splits,
                                                                          w.p.chunk, window, s);
      });
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_bf16_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                     char* buf, int len) {
  return paged::window_decode_describe<fa2d::PagedKV8, paged::kPow2G>("fa2_decode_paged_multi_window_sink_bf16_fp8_mfma", paged::kSinksOptional,
                                                                      {B, T, Hq, Hkv, max_pages, page, D, window}, buf, len);
}
