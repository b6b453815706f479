// Compile unit of the sparse multi-head latent attention (MLA) decode for a packed batch over a paged latent cache in bf16:
// cln_fa2_decode_paged_mla_sparse_varlen_bf16_plan / cln_fa2_decode_paged_mla_sparse_varlen_bf16 /
// cln_fa2_decode_paged_mla_sparse_varlen_bf16_describe (include/cln_amd_ext.h; kernel: flash_attn_decode_paged_mla_sparse_varlen_bf16.cuh;
// DESIGN 4.4.25). The plan is paged::mla_sparse_varlen_plan: paged::mla_sparse_plan with total_q in the place of B T. The checking order
// and the status codes are flash_attn_decode_paged_mla_sparse_bf16.hip's: the scale first (required, finite, > 0: -1), then
// paged::decode_args with two 16-byte inputs -- the pointers, cu_q and indices among the 4-byte aligned int inputs, behind seqlens in that
// order -- then P, the shape (a non-positive B or total_q: -1) and the plan, the workspace.
#include "flash_attn_decode_paged_mla_sparse_varlen_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2b::mlasv::kDc == paged::kMlaDc && fa2b::mlasv::kDk == paged::kMlaDk, "paged::mla_sparse_plan sizes the workspace for this kernel's value dims");
static_assert(fa2b::mlasv::kKeyStep == paged::kMlaKeyStep && fa2b::mlasv::kHeadGroup == paged::kMlaRowGroup, "paged::mla_sparse_plan plans with this kernel's step and head group");
static_assert(fa2b::mlasv::kDr == paged::kMlaDr && fa2b::mlasv::kLdsBytes == 75776, "the sibling's row and its one LDS image");

CLN_API int cln_fa2_decode_paged_mla_sparse_varlen_bf16_plan(int total_q, int Hq, int topk, int max_pages, int page, int* splits, int* chunk,
                                                             long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged::mla_sparse_varlen_plan(total_q, Hq, topk, max_pages, page, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_mla_sparse_varlen_bf16(const void* q, const void* pool, const int* block_table, const int* seqlens,
                                                        const int* cu_q, const int* indices, void* o, float* lse, void* workspace,
                                                        long long workspace_bytes, int B, int total_q, int Hq, int topk, int P, int max_pages,
                                                        int page, float softmax_scale, void* stream) {
  float mult = 0.0f;
  int rc = paged::mla_scale_arg(softmax_scale, &mult);
  if (rc != CLN_OK) return rc;
  const void* in[] = {q, pool, block_table, seqlens, cu_q, indices};  // the last four: 4-byte aligned
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  rc = paged::decode_args(in, 6, {o, lse, workspace}, workspace_bytes, P,
                          paged::mla_sparse_varlen_shape(B, total_q, Hq, topk, max_pages, page, &g, &p), p, 2);
  if (rc != CLN_OK) return rc;
  const fa2b::SparseLatentVarlen kv = {(const bf16_t*)pool, block_table, indices, max_pages, g.page_shift, topk};  // the row is key and value
  return fa2b::launch_decode_paged_mla_sparse_varlen(q, kv, seqlens, cu_q, o, lse, workspace, B, total_q, Hq, p.splits, p.chunk, mult,
                                                     (hipStream_t)stream);
}

CLN_API int cln_fa2_decode_paged_mla_sparse_varlen_bf16_describe(int B, int total_q, int Hq, int topk, int max_pages, int page,
                                                                 float softmax_scale, char* buf, int len) {
  float mult = 0.0f;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc =
      paged::mla_describe_args(buf, len, softmax_scale, &mult, paged::mla_sparse_varlen_shape(B, total_q, Hq, topk, max_pages, page, &g, &p));
  if (rc != CLN_OK) return rc;
  const int HG = (Hq + paged::kMlaRowGroup - 1) / paged::kMlaRowGroup;
  int n = snprintf(buf, len,
                   "fa2_decode_paged_mla_sparse_varlen_bf16_mfma<Dk=%d,Dv=%d> softmax_scale=%.9g (the caller's), score multiplier x log2(e) = "
                   "%.9g; B=%d total_q=%d Hq=%d topk=%d S=%d C=%d page=%d: %lld workgroups of 4 waves, one per (packed row, group of %d heads, "
                   "split of C index slots; %d head groups), a wave per 16-head tile (%d of the last group's 4 waves own rows); packed row r is "
                   "token t = r - cu_q[b] of the sequence b with cu_q[b] <= r < cu_q[b + 1], found by binary search over the device-side "
                   "offsets (clamped to [0, total_q]); a slot is valid iff 0 <= idx < vis(r) = clamp(seqlens[b], 0, max_pages page) - (T_b - 1 "
                   "- t), T_b = cu_q[b + 1] - cu_q[b]; a row of no sequence has vis = 0 without a length read: no table entry or pool row "
                   "addressed, O = 0, LSE = -inf; from there the body of fa2_decode_paged_mla_sparse_bf16_mfma: per %d-slot step the 4 waves "
                   "resolve index -> block table entry -> latent row [c %d | k_pe %d], the index fetched two steps and the table entry one step "
                   "ahead of the row, an empty slot never addressed (zeros), into one LDS image (%d bytes static, row stride %d bytes) that "
                   "feeds both products: S^T = K Q^T over all %d dims (72 MFMAs per wave and step) and O^T = V^T P^T from transposing reads of "
                   "dims 0 ... %d of the same rows (64 MFMAs) on v_mfma_f32_16x16x32_bf16, fp32 scores and accumulators, the mask by select on "
                   "64 validity flags that travel in the pad bytes of LDS rows 0 and 1, a step without a valid slot skipped, online softmax, P "
                   "and O rounded once to bf16, a token without a valid slot O = 0, LSE = -inf",
                   paged::kMlaDk, paged::kMlaDc, (double)softmax_scale, (double)mult, B, total_q, Hq, topk, p.splits, p.chunk, page,
                   (long long)total_q * HG * p.splits, paged::kMlaRowGroup, HG, (Hq - (HG - 1) * paged::kMlaRowGroup + 15) / 16,
                   fa2b::mlasv::kKeyStep, paged::kMlaDc, paged::kMlaDr, fa2b::mlasv::kLdsBytes, fa2b::mlasv::kRowBytes, paged::kMlaDk,
                   paged::kMlaDc - 1);
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; every split of every row writes its partial (an empty one m = -inf, l = 0, O = 0), then fa2_decode_combine_bf16_all<D=%d> "
                  "merges all %d splits of a query row by log-sum-exp in ascending order (workspace %lld bytes)", paged::kMlaDc, p.splits,
                  p.ws_bytes);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic");
  return n < len ? n : len - 1;
}
