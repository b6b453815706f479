// Compile unit of the sparse multi-head latent attention (MLA) decode over a paged latent cache in DeepSeek-V3.2's own FP8 row of 656 bytes
// (512 e4m3fn codes, 4 fp32 tile scales, 64 bf16 of k_pe) with bf16 queries: cln_fa2_decode_paged_mla_sparse_bf16_fp8_tile_plan /
// cln_fa2_decode_paged_mla_sparse_bf16_fp8_tile / cln_fa2_decode_paged_mla_sparse_bf16_fp8_tile_describe (include/cln_amd_ext.h; kernel:
// flash_attn_decode_paged_mla_sparse_bf16_fp8_tile.cuh, PACKED = false). The plan is the bf16 sparse entry's,
// paged::mla_sparse_plan, unchanged. The checking order and the status codes are flash_attn_decode_paged_mla_sparse_bf16_fp8.hip's without
// kv_scale -- the scales live in the rows: the softmax scale first (-1), then paged::decode_args with two 16-byte inputs, block_table,
// seqlens and indices 4-byte aligned, then P, the plan, the workspace.
//
// Built without packed fp32 ops (_build.py EXTRA_FLAGS). The reason: with them on the kernel compiles to 424 registers and SPILLS 6 VGPRs;
// without them to 412 and no spill, the condition of tests/test_no_spills.py. The flag is unit-wide, so the staging products AND the
// `acc[db] *= alpha` rescale of the loop are plain v_mul_f32 (128 a wave and step where the siblings have 64 v_pk_mul_f32): DESIGN 4.4.26.
#include "flash_attn_decode_paged_mla_sparse_bf16_fp8_tile.cuh"
#include "paged_entry.h"

static_assert(fa2b::mlast::kDc == paged::kMlaDc && fa2b::mlast::kDk == paged::kMlaDk, "paged::mla_sparse_plan sizes the workspace for this kernel's value dims");
static_assert(fa2b::mlast::kKeyStep == paged::kMlaKeyStep && fa2b::mlast::kHeadGroup == paged::kMlaRowGroup, "paged::mla_sparse_plan plans with this kernel's step and head group");
static_assert(fa2b::mlast::kDr == paged::kMlaDr && fa2b::mlast::kLdsBytes == 75776 && fa2b::mlast::kPoolRowBytes == paged::kMlaTileRowBytes, "the siblings' row and their one LDS image; the pool row of the append");

CLN_API int cln_fa2_decode_paged_mla_sparse_bf16_fp8_tile_plan(int B, int T, int Hq, int topk, int max_pages, int page, int* splits, int* chunk,
                                                               long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(paged::mla_sparse_plan(B, T, Hq, topk, max_pages, page, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_mla_sparse_bf16_fp8_tile(const void* q, const void* pool, const int* block_table, const int* seqlens,
                                                          const int* indices, void* o, float* lse, void* workspace, long long workspace_bytes,
                                                          int B, int T, int Hq, int topk, int P, int max_pages, int page, float softmax_scale,
                                                          void* stream) {
  float mult = 0.0f;
  int rc = paged::mla_scale_arg(softmax_scale, &mult);
  if (rc != CLN_OK) return rc;
  const void* in[] = {q, pool, block_table, seqlens, indices};  // the last three: 4-byte aligned
  fa2d::PagedGeometry g;
  fa2d::Plan p = {};
  rc = paged::decode_args(in, 5, {o, lse, workspace}, workspace_bytes, P, paged::mla_sparse_plan(B, T, Hq, topk, max_pages, page, &g, &p), p, 2);
  if (rc != CLN_OK) return rc;
  const fa2b::SparseLatentTile kv = {(const unsigned char*)pool, block_table, indices, max_pages, g.page_shift, topk};  // the row is key and value
  return fa2b::launch_decode_paged_mla_sparse_fp8_tile<false>(q, kv, seqlens, nullptr, o, lse, workspace, B, T, Hq, p.splits, p.chunk, mult,
                                                              (hipStream_t)stream);
}

CLN_API int cln_fa2_decode_paged_mla_sparse_bf16_fp8_tile_describe(int B, int T, int Hq, int topk, int max_pages, int page, float softmax_scale,
                                                                   char* buf, int len) {
  float mult = 0.0f;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = paged::mla_describe_args(buf, len, softmax_scale, &mult, paged::mla_sparse_plan(B, T, Hq, topk, max_pages, page, &g, &p));
  if (rc != CLN_OK) return rc;
  const int HG = (Hq + paged::kMlaRowGroup - 1) / paged::kMlaRowGroup;
  paged::Text t = {buf, len, 0};
  t.add("fa2_decode_paged_mla_sparse_bf16_fp8_tile_mfma<PACKED=0,Dk=%d,Dv=%d> softmax_scale=%.9g (the caller's), score multiplier x log2(e) = "
        "%.9g alone (the scales live in the rows); T=%d Hq=%d topk=%d S=%d C=%d page=%d: %lld workgroups of 4 waves, one per (sequence, query "
        "token, group of %d heads, split of C index slots; %d head groups), a wave per 16-head tile (%d of the last group's 4 waves own rows); ",
        paged::kMlaDk, paged::kMlaDc, (double)softmax_scale, (double)mult, T, Hq, topk, p.splits, p.chunk, page, (long long)B * T * HG * p.splits,
        paged::kMlaRowGroup, HG, (Hq - (HG - 1) * paged::kMlaRowGroup + 15) / 16);
  paged::mla_tile_describe_body(&t, "a slot valid iff 0 <= idx < vis(b, t)", p);
  return t.end();
}
