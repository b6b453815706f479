// Compile unit of the bf16 multi-token paged decode attention entries at head dim 256 (sliding window, attention sinks, any group size
// G = Hq / Hkv in 1 ... 16, softmax scale, logit soft-capping): cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan /
// cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16 / cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_describe
// (include/cln_amd_ext.h; kernel: flash_attn_decode_paged_multi_window_sink_softcap_anyg_d256_bf16.cuh): the bf16 softcap entry at
// D = 256 and no other head dim, T in 1 ... 8 with T G <= 32. The plan is this kernel's own: paged::multi_window_plan_anyg_d256, fa2d::split_plan
// on the 64-key step and D = 256. The plan entry, the checks and their order are paged::window_plan_entry / window_decode (paged_entry.h); the
// text is this unit's own: its head names MT, and its LDS and MFMA clauses have no counterpart in the siblings' text.
#include "flash_attn_decode_paged_multi_window_sink_softcap_anyg_d256_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2b::kKeyStep256 == paged::kKeyStepD256, "paged::multi_window_plan_anyg_d256 plans with the key step of this kernel");

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D,
                                                                               int window, int* splits, int* chunk, long long* workspace_bytes) {
  return paged::window_plan_entry<paged::kAnyGD256>({B, T, Hq, Hkv, max_pages, page, D, window}, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(const void* q, const void* k_pages, const void* v_pages,
                                                                          const int* block_table, const int* seqlens, const float* sinks, void* o,
                                                                          float* lse, void* workspace, long long workspace_bytes, int B, int T,
                                                                          int Hq, int Hkv, int P, int max_pages, int page, int D, int window,
                                                                          float softmax_scale, float softcap, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, sinks};
  const hipStream_t s = (hipStream_t)stream;
  return paged::window_decode<fa2b::PagedKV, paged::kAnyGD256>(
      in, sinks ? 6 : 5, o, lse, workspace, workspace_bytes, P, {B, T, Hq, Hkv, max_pages, page, D, window, softmax_scale, softcap},
      [&](auto, auto mt, auto cap, const fa2b::PagedKV& kv, const paged::WindowLaunch& w) {
        return fa2b::launch_decode_paged_multi_window_sink_softcap_anyg_d256<mt(), cap()>(
            q, kv, seqlens, sinks, o, lse, workspace, B, T, w.g.group, w.p.splits, w.p.chunk, window, w.sc.mult, w.sc.pre, w.sc.cap2, s);
      });
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D,
                                                                                   int window, float softmax_scale, float softcap, char* buf,
                                                                                   int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  paged::SoftCap sc;
  int rc = paged::softcap_arg(softmax_scale, softcap, D, &sc);
  if (rc != CLN_OK) return rc;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  rc = paged::multi_window_plan_anyg_d256(B, T, Hq, Hkv, max_pages, page, D, window, &g, &p);
  if (rc != CLN_OK) return rc;
  const int tiles = paged::multi_tiles(T, g);
  int n = snprintf(buf, len, "fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_mfma<D=%d,MT=%d,CAP=%d> softmax_scale=%.9g (%s), score "
                   "multiplier x log2(e) = %.9g; ", D, tiles, sc.cap ? 1 : 0, softmax_scale != 0.0f ? (double)softmax_scale : 1.0 / sqrt((double)D),
                   softmax_scale != 0.0f ? "the caller's" : "the default 1 / sqrt(D)", (double)sc.mult);
  if (n < len && sc.cap)
    n += snprintf(buf + n, len - n,
                  "softcap=%.9g: every score is cap tanh(q.k x / cap) in fp32, capped before the window and causal mask (a hidden key is -inf, "
                  "not -cap), the sink neither scaled nor capped; ", (double)softcap);
  if (n < len)
    n += snprintf(buf + n, len - n,
                  "T=%d G=%d W=%d span=%lld S=%d C=%d page=%d: the S splits of C keys divide the span from base = align_down(max(0, len - T - W + "
                  "1), %lld) on, no table entry and no row below base; 4 waves split the %d-key steps, one 16-key block and one K / V row per lane "
                  "and step, K rows through the block table straight to MFMA fragments, V rows through a transposed LDS read (%d bytes of V image "
                  "inside %d bytes of static LDS, which the final merge of the four waves reuses), each row loaded once for the %d query rows "
                  "(T x G, %d tiles of 16, T G <= %d) of its KV head, S^T = K Q^T (8 MFMAs per tile) and O^T = V^T P^T (16 per tile, 16 of the 32 "
                  "k-slots filled) on v_mfma_f32_16x16x32_bf16, fp32 scores and accumulators, window and causal mask by select, online softmax, P "
                  "and O rounded once to bf16",
                  T, g.group, window, paged::multi_window_span_d256(T, page, window, g.Nmax), p.splits, p.chunk, page,
                  paged::multi_window_unit_d256(page), fa2b::kKeyStep256, fa2b::kDecode256VBytes, fa2b::kDecode256LdsBytes, T * g.group, tiles,
                  paged::kMaxRowsD256);
  if (p.splits == 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; the sink of a row's head (fp32, natural log, unscaled; none when sinks is NULL) is folded into the fp32 (m, l) of the finished "
                  "row at its final store, once, and a row that sees no key stays O = 0, LSE = -inf");
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; then fa2_decode_combine_window_sink_bf16_rows<D=%d> merges the live splits ceil((len - base) / C) of a query row by log-sum-exp "
                  "in ascending order (workspace %lld bytes) and folds the sink of the row's head (none when sinks is NULL: "
                  "fa2_decode_combine_window_bf16_rows<D=%d> then) into the merged fp32 (m, l), once: the splits store raw partials, and a row "
                  "that sees no key stays O = 0, LSE = -inf",
                  D, p.ws_bytes, D);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic");
  return n < len ? n : len - 1;
}
