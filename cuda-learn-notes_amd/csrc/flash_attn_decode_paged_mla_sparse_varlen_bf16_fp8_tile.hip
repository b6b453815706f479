// Compile unit of the sparse multi-head latent attention (MLA) decode for a packed batch over a paged latent cache in DeepSeek-V3.2's own
// FP8 row of 656 bytes with bf16 queries: cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile_plan /
// cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile / cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile_describe
// (include/cln_amd_ext.h; kernel: flash_attn_decode_paged_mla_sparse_bf16_fp8_tile.cuh, PACKED = true -- the one body of the fixed-T entry
// behind the prologue of dsa_varlen_row.cuh). The plan is the bf16 packed entry's, paged::mla_sparse_varlen_plan. The
// checking order and the status codes are flash_attn_decode_paged_mla_sparse_varlen_bf16_fp8.hip's without kv_scale: the softmax scale
// first (-1), then paged::decode_args with two 16-byte inputs, block_table, seqlens, cu_q and indices 4-byte aligned, then P, the shape (a
// non-positive B or total_q: -1) and the plan, the workspace.
//
// Built without packed fp32 ops (_build.py EXTRA_FLAGS). The reason: with them on the kernel compiles to 424 registers and SPILLS 6 VGPRs;
// without them to 412 and no spill, the condition of tests/test_no_spills.py. The flag is unit-wide, so the staging products AND the
// `acc[db] *= alpha` rescale of the loop are plain v_mul_f32 (128 a wave and step where the siblings have 64 v_pk_mul_f32): DESIGN 4.4.26.
#include "flash_attn_decode_paged_mla_sparse_bf16_fp8_tile.cuh"
#include "paged_entry.h"

static_assert(fa2b::mlast::kDc == paged::kMlaDc && fa2b::mlast::kDk == paged::kMlaDk, "paged::mla_sparse_plan sizes the workspace for this kernel's value dims");
static_assert(fa2b::mlast::kKeyStep == paged::kMlaKeyStep && fa2b::mlast::kHeadGroup == paged::kMlaRowGroup, "paged::mla_sparse_plan plans with this kernel's step and head group");
static_assert(fa2b::mlast::kDr == paged::kMlaDr && fa2b::mlast::kLdsBytes == 75776 && fa2b::mlast::kPoolRowBytes == paged::kMlaTileRowBytes, "the siblings' row and their one LDS image; the pool row of the append");

CLN_API int cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile_plan(int total_q, int Hq, int topk, int max_pages, int page, int* splits,
                                                                      int* chunk, long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged::mla_sparse_varlen_plan(total_q, Hq, topk, max_pages, page, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile(const void* q, const void* pool, const int* block_table, const int* seqlens,
                                                                 const int* cu_q, const int* indices, void* o, float* lse, void* workspace,
                                                                 long long workspace_bytes, int B, int total_q, int Hq, int topk, int P,
                                                                 int max_pages, int page, float softmax_scale, void* stream) {
  float mult = 0.0f;
  int rc = paged::mla_scale_arg(softmax_scale, &mult);
  if (rc != CLN_OK) return rc;
  const void* in[] = {q, pool, block_table, seqlens, cu_q, indices};  // the last four: 4-byte aligned
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  rc = paged::decode_args(in, 6, {o, lse, workspace}, workspace_bytes, P,
                          paged::mla_sparse_varlen_shape(B, total_q, Hq, topk, max_pages, page, &g, &p), p, 2);
  if (rc != CLN_OK) return rc;
  const fa2b::SparseLatentTile kv = {(const unsigned char*)pool, block_table, indices, max_pages, g.page_shift, topk};  // the row is key and value
  return fa2b::launch_decode_paged_mla_sparse_fp8_tile<true>(q, kv, seqlens, cu_q, o, lse, workspace, B, total_q, Hq, p.splits, p.chunk, mult,
                                                             (hipStream_t)stream);
}

CLN_API int cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile_describe(int B, int total_q, int Hq, int topk, int max_pages, int page,
                                                                          float softmax_scale, char* buf, int len) {
  float mult = 0.0f;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc =
      paged::mla_describe_args(buf, len, softmax_scale, &mult, paged::mla_sparse_varlen_shape(B, total_q, Hq, topk, max_pages, page, &g, &p));
  if (rc != CLN_OK) return rc;
  const int HG = (Hq + paged::kMlaRowGroup - 1) / paged::kMlaRowGroup;
  paged::Text t = {buf, len, 0};
  t.add("fa2_decode_paged_mla_sparse_bf16_fp8_tile_mfma<PACKED=1,Dk=%d,Dv=%d> softmax_scale=%.9g (the caller's), score multiplier x log2(e) = "
        "%.9g alone (the scales live in the rows); B=%d total_q=%d Hq=%d topk=%d S=%d C=%d page=%d: %lld workgroups of 4 waves, one per (packed "
        "row, group of %d heads, split of C index slots; %d head groups), a wave per 16-head tile (%d of the last group's 4 waves own rows); "
        "packed row r is token t = r - cu_q[b] of the sequence b with cu_q[b] <= r < cu_q[b + 1], found by binary search over the device-side "
        "offsets (clamped to [0, total_q]); a row of no sequence has vis = 0 without a length read: no table entry or pool row addressed, O = "
        "0, LSE = -inf; from there the one body of the fixed-T entry: ",
        paged::kMlaDk, paged::kMlaDc, (double)softmax_scale, (double)mult, B, total_q, Hq, topk, p.splits, p.chunk, page,
        (long long)total_q * HG * p.splits, paged::kMlaRowGroup, HG, (Hq - (HG - 1) * paged::kMlaRowGroup + 15) / 16);
  paged::mla_tile_describe_body(&t, "a slot valid iff 0 <= idx < vis(r) = clamp(seqlens[b], 0, max_pages page) - (T_b - 1 - t), T_b = cu_q[b + 1] - cu_q[b]", p);
  return t.end();
}
