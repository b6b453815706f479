// The prologue of the packed ("varlen") DSA entries (cln_mla_index_logits_paged_varlen_bf16[_fp8], cln_mla_index_topk_varlen,
// cln_fa2_decode_paged_mla_sparse_varlen_bf16[_fp8]; include/cln_amd_ext.h): which sequence a packed row belongs to. One
// definition, included by all five kernels.
//
// Packed row r < total_q belongs to the largest b in [0, B) with cu_q[b] <= r; c0 = cu_q[b], T_b = cu_q[b + 1] - c0, t = r - c0. The offsets
// are read through the family's clamp (kv_append_paged_varlen.cuh): every value to [0, total_q], T_b = max(., 0), the search over the clamped
// values -- a malformed cu_q (decreasing, negative, past total_q) is outside the contract and can still name no row but r itself. The search
// is ceil(log2(B + 1)) dependent loads whose every operand is workgroup-uniform (r comes from blockIdx), the results through
// v_readfirstlane so that what follows is scalar.
//
// A row in front of cu_q[0], at or behind cu_q[B], or with t >= T_b belongs to no sequence: b = -1, and the caller reads no length, no table
// entry and no pool row for it.
#pragma once
#include <hip/hip_runtime.h>

namespace dsav {

struct PackedRow {
  int b;  // the sequence, or -1: the row belongs to none
  int t;  // the token of the sequence, 0 <= t < T
  int T;  // the tokens of the sequence in this step
};

__device__ __forceinline__ int clamped_offset(const int* __restrict__ cu_q, int i, int total_q) { return min(max(cu_q[i], 0), total_q); }

__device__ __forceinline__ PackedRow packed_row(const int* __restrict__ cu_q, int B, int total_q, unsigned r) {
  int lo = 0, hi = B;  // offset <= r for every probed b < lo, > r for every probed b >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)clamped_offset(cu_q, mid, total_q) <= r)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int b = __builtin_amdgcn_readfirstlane(lo - 1);
  if (b < 0) return {-1, 0, 0};  // a row in front of the first sequence
  const int c0 = __builtin_amdgcn_readfirstlane(clamped_offset(cu_q, b, total_q));  // <= r: b was probed
  const int T = __builtin_amdgcn_readfirstlane(max(clamped_offset(cu_q, b + 1, total_q) - c0, 0));
  const unsigned t = r - (unsigned)c0;
  if (t >= (unsigned)T) return {-1, 0, 0};  // a row behind the last sequence (or, with malformed offsets, in a gap)
  return {b, (int)t, T};
}

}  // namespace dsav
