// Compile unit of the exact top-k of DeepSeek-V3.2's indexer: cln_mla_index_topk / cln_mla_index_topk_describe (include/cln_amd_ext.h;
// kernel: mla_index_topk.cuh). Status, in this order: a missing or misaligned pointer (all three 4-byte aligned) or indices
// equal to an input (-1); paged::index_topk_shape -- a non-positive B, T, ld or topk (-1), ld >= 2^31, B T >= 2^31, topk B T past 2^61 or a
// grid that does not fit (-2).
#include "mla_index_topk.cuh"
#include "paged_entry.h"

static_assert(idxk::kThreads == paged::kTopkThreads && idxk::kBlock == paged::kTopkBlock, "paged::index_topk_shape sizes the grid for this kernel");

CLN_API int cln_mla_index_topk(const float* logits, const int* seqlens, int* indices, int B, int T, long long ld, int topk, void* stream) {
  const void* const in[] = {logits, seqlens};
  const int al16[] = {0, 0};
  int rc = paged::index_args(in, al16, 2, indices, 4);
  if (rc != CLN_OK) return rc;
  long long tokens = 0;
  rc = paged::index_topk_shape(B, T, ld, topk, &tokens);
  if (rc != CLN_OK) return rc;
  return idxk::launch_mla_index_topk(logits, seqlens, indices, T, ld, topk, tokens, (hipStream_t)stream);
}

CLN_API int cln_mla_index_topk_describe(int B, int T, long long ld, int topk, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  long long tokens = 0;
  const int rc = paged::index_topk_shape(B, T, ld, topk, &tokens);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "mla_index_topk_rows T=%d ld=%lld topk=%d: one launch, no workspace, no global atomics, no sort; %lld workgroups of %d "
                         "threads, one per (sequence, query token) row; n = max(clamp(seqlens[b], 0, ld) - (T - 1 - t), 0); n <= topk: the dense "
                         "list 0 ... n - 1 then -1; otherwise a radix select over the keys (sign bit set: complemented, else the sign bit set; -0 "
                         "as +0; a NaN by its bit pattern), 4 passes of 8 bits with a 256-bin LDS histogram and a wave scan, finds the threshold "
                         "key and how many of its ties are taken, then one ordered pass in ascending blocks of %d positions (4 a thread, one "
                         "4-byte aligned dwordx4 load) selects key > threshold, or == threshold with tie rank below the remainder, and ranks the "
                         "selected positions by a workgroup prefix sum (8 ballots, 2 counts per wave in LDS, one barrier a block): the list is "
                         "the topk first under (logit descending, position ascending), written in ascending position order, every slot written; "
                         "only logits[b, t, 0 ... n - 1] read, 5 times; %d bytes of LDS static; deterministic",
                         T, ld, topk, tokens, paged::kTopkThreads, paged::kTopkBlock, idxk::kLdsBytes);
  return n < len ? n : len - 1;
}
