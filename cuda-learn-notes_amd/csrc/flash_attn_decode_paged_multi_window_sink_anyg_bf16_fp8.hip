// Compile unit of the sliding-window multi-token paged decode attention entries with attention sinks, bf16 queries and FP8 pools, for any group
// size G = Hq / Hkv in 1 ... 16: cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan / cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8 /
// cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_describe (include/cln_amd_ext.h; kernel:
// flash_attn_decode_paged_multi_window_sink_anyg_bf16_fp8.cuh). The plan is paged::multi_window_plan_anyg, as in
// flash_attn_decode_paged_multi_window_sink_anyg_bf16.hip: neither the pools' element size nor the sink changes the splits or the workspace. The
// checks and the status codes are those of flash_attn_decode_paged_multi_window_sink_bf16_fp8.hip, argument by argument.
#include "flash_attn_decode_paged_multi_window_sink_anyg_bf16_fp8.cuh"
#include "paged_entry.h"

static_assert(fa2b::kMultiKeyStep == fa2pm::kKeyStep, "paged::multi_window_plan_anyg plans with the key step of this kernel");
static_assert(paged::kMaxRowsAnyG == 4 * 16, "paged::for_row_tiles has 1 ... 4 row tiles of 16");

CLN_API int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window,
                                                                      int* splits, int* chunk, long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged::multi_window_plan_anyg(B, T, Hq, Hkv, max_pages, page, D, window, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8(const void* q, const void* k_pages, const void* v_pages, const int* block_table,
                                                                 const int* seqlens, const float* k_scale, const float* v_scale,
                                                                 const float* sinks, void* o, float* lse, void* workspace,
                                                                 long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages,
                                                                 int page, int D, int window, void* stream) {
  const void* in[] = {q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, sinks};  // the last five: 4-byte aligned; sinks only when given
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  const int rc = paged::decode_args(in, sinks ? 8 : 7, {o, lse, workspace}, workspace_bytes, P,
                                    paged::multi_window_plan_anyg(B, T, Hq, Hkv, max_pages, page, D, window, &g, &p), p);
  if (rc != CLN_OK) return rc;
  const fa2d::PagedKV8 kv = {(const uint8_t*)k_pages, (const uint8_t*)v_pages, k_scale, v_scale, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::for_head_dim(D, [&](auto d) {
    return paged::for_row_tiles(paged::multi_tiles(T, g), [&](auto mt) {
      return fa2b::launch_decode_paged_multi_window_sink_anyg_fp8<d(), mt()>(q, kv, seqlens, sinks, o, lse, workspace, B, T, g.group, p.splits,
                                                                             p.chunk, window, s);
    });
  });
}

CLN_API int cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D,
                                                                          int window, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = paged::multi_window_plan_anyg(B, T, Hq, Hkv, max_pages, page, D, window, &g, &p);
  if (rc != CLN_OK) return rc;
  const int tiles = paged::multi_tiles(T, g);
  int n = snprintf(buf, len,
                   "fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_mfma<D=%d,MT=%d> T=%d G=%d W=%d span=%lld S=%d C=%d page=%d: the S splits of C "
                   "keys divide the span from base = align_down(max(0, len - T - W + 1), %lld) on, no table entry and no row below base; 4 waves "
                   "split the %d-key steps, e4m3 K and V rows through the block table to registers, 16 bytes per lane, converted to bf16 once "
                   "(v_cvt_scalef32_pk_bf16_fp8, exact): K to MFMA fragments, V through a transposed LDS read, each row loaded once for the %d "
                   "query rows (T x G, %d tiles of 16; (t, g) = (r / G, r mod G) by division outside the key loop, any G in 1 ... %d with T G <= "
                   "%d) of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, fp32 scores times k_scale, window and causal "
                   "mask by select, online softmax, the partial times v_scale",
                   D, tiles, T, g.group, window, paged::multi_window_span(T, page, window, g.Nmax), p.splits, p.chunk, page,
                   paged::multi_window_unit(page), fa2b::kMultiKeyStep, T * g.group, tiles, paged::kMaxGroupAnyG, paged::kMaxRowsAnyG);
  if (p.splits == 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; the sink of a row's head (fp32, natural log, unscaled; none when sinks is NULL) is folded into the fp32 (m, l) of the finished "
                  "row at its final store, once, and a row that sees no key stays O = 0, LSE = -inf");
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; then fa2_decode_combine_window_sink_bf16_rows<D=%d> merges the live splits ceil((len - base) / C) of a query row by log-sum-exp "
                  "in ascending order (workspace %lld bytes) and folds the sink of the row's head (fp32, natural log, unscaled; none when sinks is "
                  "NULL: fa2_decode_combine_window_bf16_rows<D=%d> then) into the merged fp32 (m, l), once: the splits store raw partials, and a row "
                  "that sees no key stays O = 0, LSE = -inf",
                  D, p.ws_bytes, D);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic");
  return n < len ? n : len - 1;
}
