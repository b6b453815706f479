// Gather out of a paged LATENT cache held in FP8 (OCP e4m3fn) into a PACKED batch of bf16 rows (cln_kv_gather_paged_mla_bf16_fp8,
// include/cln_amd_ext.h): kva::kv_gather_paged_mla_bf16_rows (kv_gather_paged_mla_bf16.cuh) with the dequantising load. Packed
// row cu_k[b] + i of out bf16 [total_k, 576] receives cache row starts[b] + i of sequence b (starts null: 0), i < cu_k[b + 1] - cu_k[b]; each
// element is bf16_rne(fp32(code) * kv_scale): the code converted exactly (fa2b::e4m3x8_to_b8: v_cvt_scalef32_pk_bf16_fp8 at scale 2^0, then
// bf16 -> fp32), one fp32 product with kv_scale (fp32 [1] on the device), one rounding. It is what lets the context-chunk loop of the prompt
// path run over an FP8 pool unchanged: gather -> kv_b_proj -> prefill -> merge. The launch shape, the binary search, the clamping, the zeros for
// a cache row below 0, at or past max_pages page or behind a table entry outside [0, P), and the untouched rows of no sequence are the sibling's;
// a thread moves 8 elements: 8 bytes in, 16 bytes out.
#pragma once
#include "flash_attn_paged_bf16_fp8_rows.cuh"  // e4m3x8_to_b8
#include "kv_append_paged_mla_bf16.cuh"  // kMlaDk, kThreads (the sibling gather's header defines a kernel that is no template: not included twice)

namespace kva {

struct ArgsMlaGatherBf16Fp8 {
  const uint8_t* pool;  // [P,page,576] e4m3fn
  const int *table, *starts, *cu_k;
  const float* kv_scale;  // [1]
  bf16_t* out;            // [total_k,576]
  int B, total_k, P, max_pages, page_shift;
};

__global__ __launch_bounds__(kThreads) void kv_gather_paged_mla_bf16_fp8_rows(const ArgsMlaGatherBf16Fp8 a) {
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
    if ((unsigned)pg < (unsigned)a.P) {
      const float s = a.kv_scale[0];
      const b8 c = fa2b::e4m3x8_to_b8(*(const uint2*)(a.pool + ((((size_t)pg) << a.page_shift) + ((size_t)pos & ((1u << a.page_shift) - 1u))) * kMlaDk + 8u * j));
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = (bf16_t)((float)c[e] * s);
    }
  }
  *(b8*)(a.out + (size_t)tok * kMlaDk + 8u * j) = x;
}

inline int launch_mla_gather_bf16_fp8(const ArgsMlaGatherBf16Fp8& a, long long y, hipStream_t stream) {
  CLN_LAUNCH(kv_gather_paged_mla_bf16_fp8_rows, dim3((unsigned)a.total_k, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
