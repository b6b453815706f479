// Compile unit of the bf16 sliding-window multi-token paged decode attention entries with attention sinks
// cln_fa2_decode_paged_multi_window_sink_bf16_plan / cln_fa2_decode_paged_multi_window_sink_bf16 / cln_fa2_decode_paged_multi_window_sink_bf16_describe
// (include/cln_amd_ext.h; kernels: flash_attn_decode_paged_multi_window_sink_bf16.cuh): bf16 pools, G a power of two; sinks is one more required
// input behind seqlens and changes neither the splits nor the workspace. The plan, the checks, their order and the text are
// paged::window_plan_entry / window_decode / window_decode_describe (paged_entry.h).
#include "flash_attn_decode_paged_multi_window_sink_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2b::kMultiKeyStep == fa2pm::kKeyStep, "paged::multi_window_plan plans with the key step of this kernel");

CLN_API int cln_fa2_decode_paged_multi_window_sink_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, int* splits,
                                                             int* chunk, long long* workspace_bytes) {
  return paged::window_plan_entry<paged::kPow2G>({B, T, Hq, Hkv, max_pages, page, D, window}, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                        const int* seqlens, const float* sinks, void* o, float* lse, void* workspace,
                                                        long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages, int page,
                                                        int D, int window, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, sinks};
  const hipStream_t s = (hipStream_t)stream;
  return paged::window_decode<fa2b::PagedKV, paged::kPow2G>(
      in, 6, o, lse, workspace, workspace_bytes, P, {B, T, Hq, Hkv, max_pages, page, D, window},
      [&](auto d, auto mt, auto, const fa2b::PagedKV& kv, const paged::WindowLaunch& w) {
        return fa2b::launch_decode_paged_multi_window_sink<d(), mt()>(q, kv, seqlens, sinks, o, lse, workspace, B, T, w.g.g_shift, w.p.splits,
                                                                      w.p.chunk, window, s);
      });
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                 char* buf, int len) {
  return paged::window_decode_describe<fa2b::PagedKV, paged::kPow2G>("fa2_decode_paged_multi_window_sink_bf16_mfma", paged::kSinksRequired,
                                                                     {B, T, Hq, Hkv, max_pages, page, D, window}, buf, len);
}
