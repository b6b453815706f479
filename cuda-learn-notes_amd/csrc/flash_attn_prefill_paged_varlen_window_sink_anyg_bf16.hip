// Compile unit of the bf16 sliding-window packed paged prefill attention entries with attention sinks for any group size G = Hq / Hkv in 1 ... 16
// cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16 / cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_describe (include/cln_amd_ext.h; kernel:
// flash_attn_prefill_paged_varlen_window_sink_anyg_bf16.cuh). The checks and the status codes are those of
// flash_attn_prefill_paged_varlen_window_sink_bf16.hip, argument by argument, with paged::prefill_varlen_shape_anyg for the shape; sinks, last of
// the inputs, may be null (no sink) and is checked like the others when it is not.
#include "flash_attn_prefill_paged_varlen_window_sink_anyg_bf16.cuh"
#include "paged_entry.h"

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                               const int* seqlens, const int* cu_q, const float* sinks, void* o, float* lse, int B,
                                                               int total_q, int Hq, int Hkv, int P, int max_pages, int page, int D, int window,
                                                               void* stream) {
  // 16-byte aligned up to the table, 4-byte from there on; sinks counts only when given
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, cu_q, sinks};
  int rc = paged::prefill_args(in, sinks ? 7 : 6, o, lse, P);
  if (rc != CLN_OK) return rc;
  fa2d::PagedGeometry g;
  long long slots = 0;
  rc = paged::prefill_varlen_shape_anyg(B, total_q, Hq, Hkv, max_pages, page, D, &g, &slots);
  if (rc == CLN_OK) rc = paged::window_arg(window);
  if (rc != CLN_OK) return rc;
  const fa2b::PagedKV kv = {(const bf16_t*)k_pages, (const bf16_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(D, [&](auto d) {
    return fa2b::launch_prefill_paged_varlen_window_sink_anyg<d()>(q, kv, seqlens, cu_q, sinks, o, lse, B, total_q, g.group, slots, window, s);
  });
}

CLN_API int cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D,
                                                                        int window, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  long long slots = 0;
  int rc = paged::prefill_varlen_shape_anyg(B, total_q, Hq, Hkv, max_pages, page, D, &g, &slots);
  if (rc == CLN_OK) rc = paged::window_arg(window);
  if (rc != CLN_OK) return rc;
  // the keys a tile walks at most: the window of its first token, the tokens of its rows (a tile may start inside a token when G does not
  // divide the tile: paged::prefill_tile_tokens_anyg), and the two steps its ends are aligned to
  const long long span = (long long)window + paged::prefill_tile_tokens_anyg(g.group) + 2 * fa2b::kKeyStep;
  const int n = snprintf(buf, len,
                         "fa2_prefill_paged_varlen_window_sink_anyg_bf16_mfma<D=%d> G=%d B=%d total_q=%d page=%d rows=%d keys=%d W=%d: one launch, no "
                         "workspace; %lld workgroups of 256 threads (%d KV heads x %lld slots = total_q G / %d + B, at most B of them empty), "
                         "sequence b owns the slots from cu_q[b] G / %d + b, found by binary search over the device-side offsets; a slot is a tile "
                         "of %d of the T_b G query rows t G + g of its sequence, (t, g) = (r / G, r mod G) by division outside the key loop, any "
                         "G in 1 ... %d, 32 rows per wave, and walks the keys from the step that holds the "
                         "lower edge p - W + 1 of its first token to the causal edge of its last in steps of %d, a span of at most %lld keys "
                         "whatever the length; K and V rows through the block table to LDS once per workgroup, no table entry and no row below "
                         "that first step; S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, V through ds_read_b64_tr_b16, fp32 scores, "
                         "window and causal mask by select on the steps that cross an edge, online softmax, no split over the keys (S=1, C=the "
                         "span); the sink of a row's head (fp32, natural log, unscaled; none when sinks is NULL) is folded into the fp32 (m, l) of "
                         "the finished row in the epilogue, once, and a row that sees no key stays O = 0, LSE = -inf; deterministic",
                         D, g.group, B, total_q, page, fa2b::kRowTile, fa2b::kKeyStep, window, (long long)Hkv * slots, Hkv, slots, fa2b::kRowTile,
                         fa2b::kRowTile, fa2b::kRowTile, paged::kMaxGroupAnyG, fa2b::kKeyStep, span < g.Nmax ? span : g.Nmax);
  return n < len ? n : len - 1;
}
