// The two templates that more than one compile unit of the MLA decode over the paged latent cache uses, and nothing else: the headers of those
// units define kernels that are no templates, so no second unit can include them. store_split_scaled: the FP8 pools' store (the dense and the
// sparse entry); fa2_decode_combine_bf16_all: the sparse entries' combine.
#pragma once
#include "paged_bf16.cuh"

namespace fa2b {

// store_split with kv_scale in front of the store: S = 1 the finished row (O / L) kv_scale rounded once, else the partial O kv_scale
template <int D>
__device__ __forceinline__ void store_split_scaled(const Out& out, size_t row, int t, unsigned s, int S, float mx, float L, float O, float kvs) {
  if (S == 1) {
    const float inv = L > 0.0f ? 1.0f / L : 0.0f;
    out.o[row * D + t] = (bf16_t)(O * inv * kvs);
    if (out.lse && t == 0) out.lse[row] = L > 0.0f ? (mx + __builtin_log2f(L)) * 0.6931471805599453f : FA2D_NEG_INF;
  } else {
    store_split<D>(out, row, t, s, S, mx, L, O * kvs);
  }
}

// fa2_decode_combine_bf16_rows without the liveness rule: every one of the S partials of a row was written (an empty split as (-inf, 0, 0)),
// all are merged in ascending s with the same -inf guard. One workgroup of D threads per output row.
template <int D>
__global__ __launch_bounds__(D) void fa2_decode_combine_bf16_all(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                                 bf16_t* __restrict__ o, float* __restrict__ lse, int S) {
  const unsigned row = blockIdx.x;
  const int t = threadIdx.x;
  const float* ml = ws_ml + (size_t)row * S * 2;
  const float* po = ws_o + (size_t)row * S * D + t;
  float mx = FA2D_NEG_INF;
  for (int s = 0; s < S; ++s) mx = fmaxf(mx, ml[2 * s]);
  const float ms = mx == FA2D_NEG_INF ? 0.0f : mx;  // never exp2(-inf + inf)
  float L = 0.0f, O = 0.0f;
  for (int s = 0; s < S; ++s) {
    const float f = fa2d::ex2(ml[2 * s] - ms);
    L = fmaf(ml[2 * s + 1], f, L);
    O = fmaf(po[(size_t)s * D], f, O);
  }
  store_final<D>(Out{o, lse, nullptr, nullptr}, row, t, mx, L, O);
}

}  // namespace fa2b
