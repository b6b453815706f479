// Compile unit of the logits of DeepSeek-V3.2's indexer over the paged index-key cache in bf16: cln_mla_index_logits_paged_bf16 /
// cln_mla_index_logits_paged_bf16_describe (include/cln_amd_ext.h; kernel: mla_index_logits_paged_bf16.cuh). The checking order
// and the status codes are the family's: the pointers (q_idx and idx_pool 16-byte aligned; weights, block_table, seqlens and logits 4-byte;
// the output equal to no input: -1), then P (-1), then paged::index_logits_shape -- a non-positive dimension (-1), Hi > 64, another page,
// max_pages page >= 2^31, B T >= 2^31 or a grid that does not fit (-2).
#include "mla_index_logits_paged_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2b::idx::kDim == paged::kIdxDim && fa2b::idx::kMaxHeads == paged::kIdxMaxHeads && fa2b::idx::kChunk == paged::kIdxChunk,
              "paged::index_logits_shape sizes the grid for this kernel's chunk");

CLN_API int cln_mla_index_logits_paged_bf16(const void* q_idx, const float* weights, const void* idx_pool, const int* block_table,
                                            const int* seqlens, float* logits, int B, int T, int Hi, long long ld, int P, int max_pages, int page,
                                            void* stream) {
  const void* const in[] = {q_idx, weights, idx_pool, block_table, seqlens};
  const int al16[] = {1, 0, 1, 0, 0};
  int rc = paged::index_args(in, al16, 5, logits, 4);
  if (rc != CLN_OK) return rc;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  int cap = 0, chunks = 0;
  long long wgs = 0;
  rc = paged::index_logits_shape(B, T, Hi, ld, max_pages, page, &g, &cap, &chunks, &wgs);
  if (rc != CLN_OK) return rc;
  const fa2b::IndexKeys kv = {(const bf16_t*)idx_pool, block_table, P, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return paged::pick<4, 3, 2, 1>((Hi + 15) / 16, [&](auto nhb) {
    return fa2b::launch_mla_index_logits<nhb()>(q_idx, weights, kv, seqlens, logits, T, Hi, cap, chunks, ld, wgs, s);
  });
}

CLN_API int cln_mla_index_logits_paged_bf16_describe(int B, int T, int Hi, long long ld, int max_pages, int page, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  int cap = 0, chunks = 0;
  long long wgs = 0;
  const int rc = paged::index_logits_shape(B, T, Hi, ld, max_pages, page, &g, &cap, &chunks, &wgs);
  if (rc != CLN_OK) return rc;
  const int NHB = (Hi + 15) / 16;
  const int n = snprintf(buf, len,
                         "mla_index_logits_paged_bf16_mfma<NHB=%d> T=%d Hi=%d ld=%lld cap=%d page=%d: one launch, no workspace, no LDS; %lld "
                         "workgroups of 4 waves, one per (sequence, query token, chunk of %d keys; %d chunks a token, sized from cap = min(max_pages "
                         "page, ld)), a wave per %d consecutive keys in blocks of 16; vis(b, t) = clamp(seqlens[b], 0, cap) - (T - 1 - t), a "
                         "workgroup at or past vis returns, a key or table entry at or past vis is never read; per block the index keys of %d dims "
                         "go from global memory straight into the B operand (a lane: 16 contiguous bytes of its key row per k-step, the keys of "
                         "the block after next in flight, the 16 table entries of a wave one load read back by v_readlane), S = Q K^T with the "
                         "heads as rows on v_mfma_f32_16x16x32_bf16, %d MFMAs per block (%d blocks of 16 heads x 4 k-steps, %d padding heads with "
                         "q = 0 and w = 0), fp32: acc = fma(w, max(s, 0), acc) over a lane's heads in ascending order, then the four lanes of a "
                         "key by two permlane swaps, an order that depends on neither the grid, the batch nor the length; logits[b, t, j] written "
                         "once for 0 <= j < vis and nothing else; deterministic",
                         NHB, T, Hi, ld, cap, page, wgs, paged::kIdxChunk, chunks, paged::kIdxChunk / 4, paged::kIdxDim, 4 * NHB, NHB, 16 * NHB - Hi);
  return n < len ? n : len - 1;
}
