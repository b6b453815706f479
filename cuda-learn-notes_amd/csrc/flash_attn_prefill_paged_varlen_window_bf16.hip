// Compile unit of the bf16 sliding-window packed paged prefill attention entries cln_fa2_prefill_paged_varlen_window_bf16 /
// cln_fa2_prefill_paged_varlen_window_bf16_describe (include/cln_amd_ext.h; kernel: flash_attn_prefill_paged_varlen_window_bf16.cuh): bf16 pools,
// G a power of two, no sinks. The checks, their order and the text are paged::window_prefill / window_prefill_describe (paged_entry.h).
#include "flash_attn_prefill_paged_varlen_window_bf16.cuh"
#include "paged_entry.h"

CLN_API int cln_fa2_prefill_paged_varlen_window_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                     const int* seqlens, const int* cu_q, void* o, float* lse, int B, int total_q, int Hq, int Hkv,
                                                     int P, int max_pages, int page, int D, int window, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, cu_q};
  const hipStream_t s = (hipStream_t)stream;
  return paged::window_prefill<fa2b::PagedKV, paged::kPow2G>(
      in, 6, o, lse, P, {B, total_q, Hq, Hkv, max_pages, page, D, window}, [&](auto d, auto, const fa2b::PagedKV& kv, const paged::WindowLaunch& w) {
        return fa2b::launch_prefill_paged_varlen_window<d()>(q, kv, seqlens, cu_q, o, lse, B, total_q, w.g.g_shift, w.slots, window, s);
      });
}

CLN_API int cln_fa2_prefill_paged_varlen_window_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                              char* buf, int len) {
  return paged::window_prefill_describe<fa2b::PagedKV, paged::kPow2G>("fa2_prefill_paged_varlen_window_bf16_mfma", paged::kNoSinks,
                                                                      {B, total_q, Hq, Hkv, max_pages, page, D, window}, buf, len);
}
