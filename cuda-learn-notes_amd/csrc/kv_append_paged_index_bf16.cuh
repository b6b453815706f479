// Append to the paged INDEX-KEY cache of DeepSeek-V3.2's indexer in bf16 for a PACKED batch (cln_kv_append_paged_index_bf16,
// include/cln_amd_ext.h). A pool row is one index key of 128 dims per cached token, shared by all index heads; the pool
// [P, page, 128] sits behind the block table of the latent cache. The semantics and the contract are kva::kv_append_paged_mla_bf16_rows'
// (kv_append_paged_mla_bf16.cuh): the cu_q convention, token i of sequence b at pos = seqlens[b] - T_b + i, liveness, a token that is not live
// writes nothing, rows of no sequence untouched, a table entry outside [0, P) stores nothing. There is no rotation here, on purpose: the model
// rotates the key and THEN applies a Hadamard transform before it caches it, so a rotation fused into this copy would sit in the wrong place.
//
// A copy kernel, a thread per 16-byte piece: 16 pieces a row, so a workgroup of kva::kThreads serves 16 packed rows; the sequence of a row
// by the family's binary search over the clamped offsets (per thread here: the rows of a workgroup may belong to different sequences).
#pragma once
#include "kv_append_paged.cuh"
#include "paged_bf16.cuh"

namespace kva {

constexpr int kIdxDim = 128;

struct ArgsIndexBf16 {
  const bf16_t* k_new;  // [total_q,128]
  bf16_t* pool;         // [P,page,128]
  const int *table, *seqlens, *cu_q;
  int B, total_q, P, max_pages, page_shift;
};

__global__ __launch_bounds__(kThreads) void kv_append_paged_index_bf16_rows(const ArgsIndexBf16 a) {
  constexpr unsigned PPR = kIdxDim / 8;  // pieces = threads per row
  const unsigned u = blockIdx.x * kThreads + threadIdx.x;
  const unsigned tok = u / PPR, j = u % PPR;  // the packed row and the piece
  if (tok >= (unsigned)a.total_q) return;
  // the largest b in [0, B) whose clamped offset is <= tok
  int lo = 0, hi = a.B;  // offset <= tok for every b < lo, > tok for every b >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)min(max(a.cu_q[mid], 0), a.total_q) <= tok)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int b = lo - 1;
  if (b < 0) return;  // a row in front of the first sequence
  const int c0 = min(max(a.cu_q[b], 0), a.total_q);
  const int T = max(min(max(a.cu_q[b + 1], 0), a.total_q) - c0, 0);
  const unsigned t = tok - (unsigned)c0;
  if (t >= (unsigned)T) return;  // a row behind the last sequence
  const long long pos = (long long)a.seqlens[b] - T + (long long)t;
  if (pos < 0 || pos >= ((long long)a.max_pages << a.page_shift)) return;  // not live
  const int pg = a.table[(size_t)b * a.max_pages + (size_t)(pos >> a.page_shift)];
  if ((unsigned)pg >= (unsigned)a.P) return;  // outside the caller's contract: nothing is stored rather than stored out of the pool
  bf16_t* dst = a.pool + ((((size_t)pg) << a.page_shift) + ((size_t)pos & ((1u << a.page_shift) - 1u))) * kIdxDim;
  *(b8*)(dst + 8u * j) = *(const b8*)(a.k_new + (size_t)tok * kIdxDim + 8u * j);
}

inline int launch_index_bf16(const ArgsIndexBf16& a, long long wgs, hipStream_t stream) {
  CLN_LAUNCH(kv_append_paged_index_bf16_rows, dim3((unsigned)wgs), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
