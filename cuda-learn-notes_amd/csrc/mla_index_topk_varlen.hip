// Compile unit of the exact top-k of DeepSeek-V3.2's indexer for a packed batch: cln_mla_index_topk_varlen /
// cln_mla_index_topk_varlen_describe (include/cln_amd_ext.h; kernel: mla_index_topk_varlen.cuh). Status, in this order: a
// missing or misaligned pointer (all four 4-byte aligned; cu_q behind seqlens) or indices equal to an input (-1);
// paged::index_topk_varlen_shape -- a non-positive B, total_q, ld or topk (-1), ld >= 2^31, topk total_q past 2^61 or a grid that does not
// fit (-2).
#include "mla_index_topk_varlen.cuh"
#include "paged_entry.h"

static_assert(idxkv::kThreads == paged::kTopkThreads && idxkv::kBlock == paged::kTopkBlock,
              "paged::index_topk_varlen_shape sizes the grid for this kernel");
static_assert(idxkv::kLdsBytes == 1288, "the sibling's LDS");

CLN_API int cln_mla_index_topk_varlen(const float* logits, const int* seqlens, const int* cu_q, int* indices, int B, int total_q, long long ld,
                                      int topk, void* stream) {
  const void* const in[] = {logits, seqlens, cu_q};
  const int al16[] = {0, 0, 0};
  int rc = paged::index_args(in, al16, 3, indices, 4);
  if (rc != CLN_OK) return rc;
  long long tokens = 0;
  rc = paged::index_topk_varlen_shape(B, total_q, ld, topk, &tokens);
  if (rc != CLN_OK) return rc;
  return idxkv::launch_mla_index_topk_varlen(logits, seqlens, cu_q, indices, B, total_q, ld, topk, (hipStream_t)stream);
}

CLN_API int cln_mla_index_topk_varlen_describe(int B, int total_q, long long ld, int topk, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  long long tokens = 0;
  const int rc = paged::index_topk_varlen_shape(B, total_q, ld, topk, &tokens);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "mla_index_topk_varlen_rows B=%d total_q=%d ld=%lld topk=%d: one launch, no workspace, no global atomics, no sort; %lld "
                         "workgroups of %d threads, one per packed row; packed row r is token t = r - cu_q[b] of the sequence b with cu_q[b] <= r "
                         "< cu_q[b + 1], found by binary search over the device-side offsets (clamped to [0, total_q]); n = max(clamp(seqlens[b], "
                         "0, ld) - (T_b - 1 - t), 0), T_b = cu_q[b + 1] - cu_q[b], and n = 0 without a length read for a row of no sequence; from "
                         "there the body of mla_index_topk_rows: n <= topk: the dense list 0 ... n - 1 then -1; otherwise a radix select over the "
                         "keys, 4 passes of 8 bits with a 256-bin LDS histogram and a wave scan, finds the threshold key and how many of its ties "
                         "are taken, then one ordered pass in ascending blocks of %d positions selects key > threshold, or == threshold with tie "
                         "rank below the remainder, and ranks the selected positions by a workgroup prefix sum: the list is the topk first under "
                         "(logit descending, position ascending), written in ascending position order, every slot of every row written; only "
                         "logits[r, 0 ... n - 1] read, 5 times; %d bytes of LDS static; deterministic",
                         B, total_q, ld, topk, tokens, paged::kTopkThreads, paged::kTopkBlock, idxkv::kLdsBytes);
  return n < len ? n : len - 1;
}
