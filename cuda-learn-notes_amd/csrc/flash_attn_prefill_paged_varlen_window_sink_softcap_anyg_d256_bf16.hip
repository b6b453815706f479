// Compile unit of the bf16 packed paged prefill attention entries at head dim 256 (sliding window, attention sinks, any group size G = Hq / Hkv in
// 1 ... 16, softmax scale, logit soft-capping): cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16 /
// cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_describe (include/cln_amd_ext.h; kernel:
// flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16.cuh): the bf16 softcap entry at D = 256 and no other head
// dim; softcap == 0 launches the CAP = false instantiation. The checks and their order are paged::window_prefill (paged_entry.h); the text is this
// unit's own, behind paged::softcap_describe: its LDS and register clauses have no counterpart in the siblings' text.
#include "flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2b::kHeadDim256 == paged::kHeadDim256, "one head dim");

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16(const void* q, const void* k_pages, const void* v_pages,
                                                                            const int* block_table, const int* seqlens, const int* cu_q,
                                                                            const float* sinks, void* o, float* lse, int B, int total_q, int Hq,
                                                                            int Hkv, int P, int max_pages, int page, int D, int window,
                                                                            float softmax_scale, float softcap, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, cu_q, sinks};
  const hipStream_t s = (hipStream_t)stream;
  return paged::window_prefill<fa2b::PagedKV, paged::kAnyGD256>(
      in, sinks ? 7 : 6, o, lse, P, {B, total_q, Hq, Hkv, max_pages, page, D, window, softmax_scale, softcap},
      [&](auto, auto cap, const fa2b::PagedKV& kv, const paged::WindowLaunch& w) {
        return fa2b::launch_prefill_paged_varlen_window_sink_softcap_anyg_d256<cap()>(q, kv, seqlens, cu_q, sinks, o, lse, B, total_q, w.g.group,
                                                                                      w.slots, window, w.sc.mult, w.sc.pre, w.sc.cap2, s);
      });
}

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page,
                                                                                     int D, int window, float softmax_scale, float softcap,
                                                                                     char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  paged::SoftCap sc;
  int rc = paged::softcap_arg(softmax_scale, softcap, D, &sc);
  if (rc != CLN_OK) return rc;
  fa2d::PagedGeometry g;
  long long slots = 0;
  rc = paged::window_prefill_shape<paged::kAnyGD256>({B, total_q, Hq, Hkv, max_pages, page, D, window}, &g, &slots);
  if (rc != CLN_OK) return rc;
  int n = paged::softcap_describe(buf, len, "fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_mfma", D, softmax_scale, softcap, sc, false);
  const long long span = (long long)window + paged::prefill_tile_tokens_anyg(g.group) + 2 * fa2b::kKeyStep;
  if (n < len - 1)
    n += snprintf(buf + n, len - n,
                  "G=%d B=%d total_q=%d page=%d rows=%d keys=%d W=%d: one launch, no workspace; %lld workgroups of 256 threads, one per CU "
                  "(__launch_bounds__(256, 1): a wave has the unified file of 512 registers, the accumulators in AGPRs) with %d bytes of static LDS "
                  "(K and V of a %d-key step in rows of 2 D + 32 bytes); %d KV heads x %lld slots = total_q G / %d + B, sequence b owns the slots "
                  "from cu_q[b] G / %d + b; a slot is a tile of %d of the T_b G query rows t G + g of its sequence, two 16-row tiles per wave, and "
                  "walks the keys from the step that holds the lower edge p - W + 1 of its first token to the causal edge of its last in steps of "
                  "%d, a span of at most %lld keys whatever the length; K and V rows through the block table to LDS once per workgroup, no table "
                  "entry and no row below that first step; S^T = K Q^T (64 MFMAs per wave and step) and O^T = V^T P^T (64) on "
                  "v_mfma_f32_16x16x32_bf16, V through ds_read_b64_tr_b16, fp32 scores and accumulators, window and causal mask by select on the "
                  "steps that cross an edge, online softmax, P and O rounded once to bf16, no split over the keys; the sink of a row's head is "
                  "folded into the fp32 (m, l) of the finished row in the epilogue, once, and a row that sees no key stays O = 0, LSE = -inf; "
                  "deterministic",
                  g.group, B, total_q, page, fa2b::kRowTile, fa2b::kKeyStep, window, (long long)Hkv * slots, fa2b::kPrefill256LdsBytes,
                  fa2b::kKeyStep, Hkv, slots, fa2b::kRowTile, fa2b::kRowTile, fa2b::kRowTile, fa2b::kKeyStep, span < g.Nmax ? span : g.Nmax);
  return n < len ? n : len - 1;
}
