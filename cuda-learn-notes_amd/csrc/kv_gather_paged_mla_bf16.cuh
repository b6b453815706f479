// Gather out of a paged LATENT cache in bf16 for a PACKED batch (cln_kv_gather_paged_mla_bf16, include/cln_amd_ext.h): the
// mirror of kva::kv_append_paged_mla_bf16_rows (kv_append_paged_mla_bf16.cuh). Packed row cu_k[b] + i of out [total_k, 576] receives cache row
// starts[b] + i of sequence b (starts null: 0), i < cu_k[b + 1] - cu_k[b], bit for bit: a context chunk a caller feeds to kv_b_proj without an
// index op. The launch shape is the append's without q: a packed row x the 72 16-byte pieces of its latent row; the sequence of a row by the
// same binary search over the clamped offsets. A cache row below 0 or at or past max_pages page is written as zeros and its table entry is never
// followed; so is one whose table entry lies outside [0, P) (outside the caller's contract: nothing is read out of the pool). Rows of no
// sequence are untouched.
#pragma once
#include "kv_append_paged_mla_bf16.cuh"

namespace kva {

struct ArgsMlaGatherBf16 {
  const bf16_t* pool;  // [P,page,576]
  const int *table, *starts, *cu_k;
  bf16_t* out;  // [total_k,576]
  int B, total_k, P, max_pages, page_shift;
};

__global__ __launch_bounds__(kThreads) void kv_gather_paged_mla_bf16_rows(const ArgsMlaGatherBf16 a) {
  constexpr unsigned PPR = kMlaDk / 8;  // pieces = threads per row
  const unsigned tok = blockIdx.x;      // the packed row, < total_k
  const unsigned j = blockIdx.y * kThreads + threadIdx.x;
  if (j >= PPR) return;
  // the largest b in [0, B) whose clamped offset is <= tok
  int lo = 0, hi = a.B;  // offset <= tok for every b < lo, > tok for every b >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)min(max(a.cu_k[mid], 0), a.total_k) <= tok)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int b = __builtin_amdgcn_readfirstlane(lo - 1);
  if (b < 0) return;  // a row in front of the first sequence
  const int c0 = __builtin_amdgcn_readfirstlane(min(max(a.cu_k[b], 0), a.total_k));
  const int n = __builtin_amdgcn_readfirstlane(max(min(max(a.cu_k[b + 1], 0), a.total_k) - c0, 0));
  const unsigned i = tok - (unsigned)c0;
  if (i >= (unsigned)n) return;  // a row behind the last sequence
  const long long pos = (long long)(a.starts ? a.starts[b] : 0) + (long long)i;
  b8 x = {};
  if (pos >= 0 && pos < ((long long)a.max_pages << a.page_shift)) {
    const int pg = a.table[(size_t)b * a.max_pages + (size_t)(pos >> a.page_shift)];
    if ((unsigned)pg < (unsigned)a.P)
      x = *(const b8*)(a.pool + ((((size_t)pg) << a.page_shift) + ((size_t)pos & ((1u << a.page_shift) - 1u))) * kMlaDk + 8u * j);
  }
  *(b8*)(a.out + (size_t)tok * kMlaDk + 8u * j) = x;
}

inline int launch_mla_gather_bf16(const ArgsMlaGatherBf16& a, long long y, hipStream_t stream) {
  CLN_LAUNCH(kv_gather_paged_mla_bf16_rows, dim3((unsigned)a.total_k, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
