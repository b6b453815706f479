// Compile unit of the bf16 multi-head latent attention (MLA) decode over a paged latent cache: cln_fa2_decode_paged_mla_bf16_plan /
// cln_fa2_decode_paged_mla_bf16 / cln_fa2_decode_paged_mla_bf16_describe (include/cln_amd_ext.h; kernel: flash_attn_decode_paged_mla_bf16.cuh;
// DESIGN 4.4.17). The plan is paged::mla_plan: fa2d::split_plan on B ceil(T Hq / 64) workgroup jobs, the 64-key step and D = 512. The checking
// order and the status codes: the scale first (required, finite, > 0: -1), then paged::decode_args with two 16-byte inputs -- the pointers,
// P, the plan, the workspace.
#include "flash_attn_decode_paged_mla_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2b::kMlaDc == paged::kMlaDc && fa2b::kMlaDk == paged::kMlaDk, "paged::mla_plan sizes the workspace for this kernel's value dims");
static_assert(fa2b::kMlaKeyStep == paged::kMlaKeyStep && fa2b::kMlaRowGroup == paged::kMlaRowGroup, "paged::mla_plan plans with this kernel's step and row group");

CLN_API int cln_fa2_decode_paged_mla_bf16_plan(int B, int T, int Hq, int max_pages, int page, int* splits, int* chunk,
                                               long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged::mla_plan(B, T, Hq, max_pages, page, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_mla_bf16(const void* q, const void* pool, const int* block_table, const int* seqlens, void* o, float* lse,
                                          void* workspace, long long workspace_bytes, int B, int T, int Hq, int P, int max_pages, int page,
                                          float softmax_scale, void* stream) {
  float mult = 0.0f;
  int rc = paged::mla_scale_arg(softmax_scale, &mult);
  if (rc != CLN_OK) return rc;
  const void* in[] = {q, pool, block_table, seqlens};  // the last two: 4-byte aligned
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  rc = paged::decode_args(in, 4, {o, lse, workspace}, workspace_bytes, P, paged::mla_plan(B, T, Hq, max_pages, page, &g, &p), p, 2);
  if (rc != CLN_OK) return rc;
  const fa2b::PagedKV kv = {(const bf16_t*)pool, (const bf16_t*)pool, block_table, 1, max_pages, g.page_shift};  // the row is key and value
  return fa2b::launch_decode_paged_mla(q, kv, seqlens, o, lse, workspace, B, T, Hq, p.splits, p.chunk, mult, (hipStream_t)stream);
}

CLN_API int cln_fa2_decode_paged_mla_bf16_describe(int B, int T, int Hq, int max_pages, int page, float softmax_scale, char* buf, int len) {
  float mult = 0.0f;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = paged::mla_describe_args(buf, len, softmax_scale, &mult, paged::mla_plan(B, T, Hq, max_pages, page, &g, &p));
  if (rc != CLN_OK) return rc;
  const int R = T * Hq, RG = (R + paged::kMlaRowGroup - 1) / paged::kMlaRowGroup;
  int n = snprintf(buf, len,
                   "fa2_decode_paged_mla_bf16_mfma<Dk=%d,Dv=%d> softmax_scale=%.9g (the caller's), score multiplier x log2(e) = %.9g; T=%d Hq=%d "
                   "R=%d S=%d C=%d page=%d: %lld workgroups of 4 waves, one per (sequence, split, row group of %d query rows; %d row groups), a wave "
                   "per 16-row tile (%d of the last group's 4 waves own rows); per %d-key step the 4 waves fetch the latent rows [c %d | k_pe %d] "
                   "through the block table once, a row per lane, into one LDS image (%d bytes static, row stride %d bytes) that feeds both "
                   "products: S^T = K Q^T from plain row reads over all %d dims (72 MFMAs per wave and step) and O^T = V^T P^T from transposing "
                   "reads of dims 0 ... %d of the same rows (64 MFMAs, all 32 k-slots filled) on v_mfma_f32_16x16x32_bf16, fp32 scores and "
                   "accumulators, causal mask by select, online softmax, P and O rounded once to bf16, a row that sees no key O = 0, LSE = -inf",
                   paged::kMlaDk, paged::kMlaDc, (double)softmax_scale, (double)mult, T, Hq, R, p.splits, p.chunk, page, (long long)B * RG * p.splits,
                   paged::kMlaRowGroup, RG, (R - (RG - 1) * paged::kMlaRowGroup + 15) / 16, fa2b::kMlaKeyStep, paged::kMlaDc, paged::kMlaDr,
                   fa2b::kMlaLdsBytes, fa2b::kMlaRowBytes, paged::kMlaDk, paged::kMlaDc - 1);
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; then fa2_decode_combine_bf16_rows<D=%d> merges the live splits of a query row by log-sum-exp in ascending order (workspace %lld "
                  "bytes)", paged::kMlaDc, p.ws_bytes);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic");
  return n < len ? n : len - 1;
}
