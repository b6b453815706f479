// The merge of two caller-held attention states over disjoint key sets (cln_attn_merge_states_bf16, include/cln_amd_ext.h): what
// a chunked prefill needs to join the causal part over the new tokens with the non-causal parts over the context chunks. Per row, all in fp32:
//   m = max(lse_a, lse_b);  m = -inf: O = 0, LSE = -inf;  else w = exp(lse - m) per side, a side whose LSE is -inf SELECTED out (its O may hold
//   anything, NaN included), O = (w_a O_a + w_b O_b) / (w_a + w_b) rounded once to bf16, LSE = m + ln(w_a + w_b).
// It is the arithmetic of the decode combine (fa2_decode_combine_bf16_rows) on two states in natural-log form. A thread per 16-byte piece; a
// workgroup serves whole rows (256 / (D / 8) of them) and every thread reads its row's two LSEs before the barrier in front of the one LSE
// store, so lse may be lse_a; o may be o_a because a thread reads the piece it writes. One launch, no atomics: deterministic.
#pragma once
#include "paged_bf16.cuh"

namespace attm {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void attn_merge_states_bf16_rows(const bf16_t* o_a, const float* lse_a, const bf16_t* __restrict__ o_b,
                                                                       const float* __restrict__ lse_b, bf16_t* o, float* lse, long long rows,
                                                                       int ppr, int rows_per_wg) {
  const int r = threadIdx.x / ppr, j = threadIdx.x - r * ppr;  // ppr = D / 8 pieces per row
  const long long row = (long long)blockIdx.x * rows_per_wg + r;
  const bool mine = r < rows_per_wg && row < rows;
  float la = FA2D_NEG_INF, lb = FA2D_NEG_INF;
  if (mine) la = lse_a[row], lb = lse_b[row];
  __syncthreads();  // lse may be lse_a: every thread of the row's workgroup has read it
  if (!mine) return;
  const float m = fmaxf(la, lb);
  const size_t e = ((size_t)row * ppr + j) * 8;
  if (m == FA2D_NEG_INF) {  // neither side saw a key
    *reinterpret_cast<b8*>(o + e) = b8{};
    if (lse && j == 0) lse[row] = FA2D_NEG_INF;
    return;
  }
  const bool has_a = la != FA2D_NEG_INF, has_b = lb != FA2D_NEG_INF;
  const float wa = has_a ? expf(la - m) : 0.0f, wb = has_b ? expf(lb - m) : 0.0f;
  const float ws = wa + wb;
  b8 xa = {}, xb = {}, y;
  if (has_a) xa = *reinterpret_cast<const b8*>(o_a + e);
  if (has_b) xb = *reinterpret_cast<const b8*>(o_b + e);
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = (bf16_t)((wa * (float)xa[i] + wb * (float)xb[i]) / ws);
  *reinterpret_cast<b8*>(o + e) = y;
  if (lse && j == 0) lse[row] = m + logf(ws);
}

inline int launch_merge(const void* o_a, const float* lse_a, const void* o_b, const float* lse_b, void* o, float* lse, long long rows, int D,
                        int rows_per_wg, long long wgs, hipStream_t stream) {
  CLN_LAUNCH(attn_merge_states_bf16_rows, dim3((unsigned)wgs), dim3(kThreads), 0, stream, (const bf16_t*)o_a, lse_a, (const bf16_t*)o_b, lse_b,
             (bf16_t*)o, lse, rows, D / 8, rows_per_wg);
  return cln_check_launch();
}

}  // namespace attm
