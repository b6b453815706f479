// Compile unit of the merge of two attention states: cln_attn_merge_states_bf16 / cln_attn_merge_states_bf16_describe (include/cln_amd_ext.h;
// kernel: attn_merge_states_bf16.cuh). -1 for a missing or misaligned pointer (o_a, o_b, o 16 bytes; the LSEs 4), an output that
// is an input other than its own a side (o may be o_a, lse may be lse_a), or a non-positive dimension; -2 for a D outside 8 ... 512 or no
// multiple of 8, or a grid that does not fit.
#include "attn_merge_states_bf16.cuh"
#include "paged_entry.h"

static_assert(attm::kThreads == paged::kMergeThreads, "paged::merge_shape sizes this kernel's launch");

CLN_API int cln_attn_merge_states_bf16(const void* o_a, const float* lse_a, const void* o_b, const float* lse_b, void* o, float* lse, long long rows,
                                       int D, void* stream) {
  if (!o_a || !lse_a || !o_b || !lse_b || !o) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(o_a) || !cln_aligned16(o_b) || !cln_aligned16(o) || !cln_aligned(lse_a, 4) || !cln_aligned(lse_b, 4) || !cln_aligned(lse, 4))
    return CLN_ERR_BAD_ARG;
  const void* const other[] = {o_b, lse_a, lse_b};  // what o may not be
  for (const void* p : other)
    if (o == p) return CLN_ERR_BAD_ARG;
  const void* const other_lse[] = {o_a, o_b, lse_b, o};  // what lse may not be
  for (const void* p : other_lse)
    if (lse && (const void*)lse == p) return CLN_ERR_BAD_ARG;
  int rows_per_wg = 0;
  long long wgs = 0;
  const int rc = paged::merge_shape(rows, D, &rows_per_wg, &wgs);
  if (rc != CLN_OK) return rc;
  return attm::launch_merge(o_a, lse_a, o_b, lse_b, o, lse, rows, D, rows_per_wg, wgs, (hipStream_t)stream);
}

CLN_API int cln_attn_merge_states_bf16_describe(long long rows, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int rows_per_wg = 0;
  long long wgs = 0;
  const int rc = paged::merge_shape(rows, D, &rows_per_wg, &wgs);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "attn_merge_states_bf16_rows rows=%lld D=%d: one launch, no workspace; %lld workgroups of 256 threads, %d whole rows each, a "
                         "thread per 16-byte piece (%d per row); per row in fp32 m = max(lse_a, lse_b), w = exp(lse - m) per side, a side whose LSE is "
                         "-inf selected out (its O is not read), O = (w_a O_a + w_b O_b) / (w_a + w_b) rounded once to bf16, LSE = m + ln(w_a + w_b), "
                         "both -inf: O = 0, LSE = -inf; o may be o_a and lse may be lse_a (the LSEs are read in front of a barrier); deterministic",
                         rows, D, wgs, rows_per_wg, D / 8);
  return n < len ? n : len - 1;
}
