// Compile unit of the logits of DeepSeek-V3.2's indexer for a packed batch over the paged index-key cache held in FP8 with per-token
// scales: cln_mla_index_logits_paged_varlen_bf16_fp8 / cln_mla_index_logits_paged_varlen_bf16_fp8_describe (include/cln_amd_ext.h; kernel:
// mla_index_logits_paged_varlen_bf16_fp8.cuh). The checking order and the status codes are
// mla_index_logits_paged_varlen_bf16.hip's.
#include "mla_index_logits_paged_varlen_bf16_fp8.cuh"
#include "paged_entry.h"

static_assert(fa2b::idx::kDim == paged::kIdxDim && fa2b::idx::kMaxHeads == paged::kIdxMaxHeads && fa2b::idx::kChunk == paged::kIdxChunk,
              "paged::index_logits_varlen_shape sizes the grid for this kernel's chunk");

CLN_API int cln_mla_index_logits_paged_varlen_bf16_fp8(const void* q_idx, const float* weights, const void* idx_pool, const int* block_table,
                                                       const int* seqlens, const int* cu_q, float* logits, int B, int total_q, int Hi,
                                                       long long ld, int P, int max_pages, int page, void* stream) {
  const void* const in[] = {q_idx, weights, idx_pool, block_table, seqlens, cu_q};
  const int al16[] = {1, 0, 1, 0, 0, 0};
  int rc = paged::index_args(in, al16, 6, logits, 4);
  if (rc != CLN_OK) return rc;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  int cap = 0, chunks = 0;
  long long wgs = 0;
  rc = paged::index_logits_varlen_shape(B, total_q, Hi, ld, max_pages, page, &g, &cap, &chunks, &wgs);
  if (rc != CLN_OK) return rc;
  const fa2b::IndexKeysFp8 kv = {(const uint8_t*)idx_pool, block_table, P, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::pick<4, 3, 2, 1>((Hi + 15) / 16, [&](auto nhb) {
    return fa2b::launch_mla_index_logits_varlen_fp8<nhb()>(q_idx, weights, kv, seqlens, cu_q, logits, B, total_q, Hi, cap, chunks, ld, wgs, s);
  });
}

CLN_API int cln_mla_index_logits_paged_varlen_bf16_fp8_describe(int B, int total_q, int Hi, long long ld, int max_pages, int page, char* buf,
                                                                int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  int cap = 0, chunks = 0;
  long long wgs = 0;
  const int rc = paged::index_logits_varlen_shape(B, total_q, Hi, ld, max_pages, page, &g, &cap, &chunks, &wgs);
  if (rc != CLN_OK) return rc;
  const int NHB = (Hi + 15) / 16;
  const int n = snprintf(buf, len,
                         "mla_index_logits_paged_varlen_bf16_fp8_mfma<NHB=%d> B=%d total_q=%d Hi=%d ld=%lld cap=%d page=%d: one launch, no workspace, "
                         "no LDS; %lld workgroups of 4 waves, one per (packed row, chunk of %d keys; %d chunks a row, sized from cap = "
                         "min(max_pages page, ld)), a wave per %d consecutive keys in blocks of 16; packed row r is token t = r - cu_q[b] of the "
                         "sequence b with cu_q[b] <= r < cu_q[b + 1], found by binary search over the device-side offsets (clamped to [0, "
                         "total_q]); a row of no sequence writes nothing and reads no length, table entry, key or scale; vis(r) = "
                         "clamp(seqlens[b], 0, cap) - (T_b - 1 - t), T_b = cu_q[b + 1] - cu_q[b], a workgroup at or past vis returns, a key, scale "
                         "or table entry at or past vis is never read; from there the body of mla_index_logits_paged_bf16_fp8_mfma: a page is %d "
                         "bytes: codes [%d,%d] e4m3fn, then scales [%d] fp32; per block a lane loads 32 contiguous code bytes of its key row as "
                         "two dwordx4 and the key's scale as one dword, the codes become bf16 exactly (v_cvt_scalef32_pk_bf16_fp8 at scale 1) on "
                         "the way into the B operand, S = Q C^T with the heads as rows on v_mfma_f32_16x16x32_bf16, %d MFMAs per block (%d blocks "
                         "of 16 heads x 4 k-steps, %d padding heads with q = 0 and w = 0), fp32: acc = fma(w, max(s, 0), acc) over a lane's heads "
                         "in ascending order, then the four lanes of a key by two permlane swaps, then the key's scale once (equal to "
                         "dequantise-then-ReLU for a scale >= 0: the caller's contract), an order that depends on neither the grid, the batch nor "
                         "the length; logits[r, j] written once for 0 <= j < vis and nothing else; deterministic",
                         NHB, B, total_q, Hi, ld, cap, page, wgs, paged::kIdxChunk, chunks, paged::kIdxChunk / 4, 132 * page, page, paged::kIdxDim,
                         page, 4 * NHB, NHB, 16 * NHB - Hi);
  return n < len ? n : len - 1;
}
