// The weighted combine of a mixture-of-experts layer (cln_moe_combine_bf16, include/cln_amd_ext.h): y bf16 [M_total, N] (the
// down projection's output, rows sorted by expert), pos int32 [T, k] (cln_moe_sort's: slot -> row, or -1), w fp32 [T, k], residual bf16
// [T, N] or null -> out bf16 [T, N]:
//   out[t] = bf16_rne( residual[t] + sum_j w[t, j] y[pos[t, j]] )     fp32, one fmaf a term in ascending j, one rounding
// A pos outside [0, M_total) contributes nothing (its row is not loaded and its weight not used).
//
// blockIdx.x = the token, blockIdx.y = a run of blockDim.x pieces of 8 columns; a thread owns 8 columns and loads 16 bytes a term. The k
// positions and weights of the token are loaded once per workgroup, by its first k threads into LDS; every thread then issues all its row
// loads (16 compile-time slots, the dead ones predicated off) before the first fmaf. No atomics; 128 bytes of LDS.
#pragma once
#include "paged_bf16.cuh"

namespace moe {

constexpr int kCombineMaxK = 16;

struct CombineArgs {
  const bf16_t *y, *residual;  // residual may be null
  const int* pos;
  const float* w;
  bf16_t* out;
  int M, N, k;
};

__global__ __launch_bounds__(256) void moe_combine_rows(const CombineArgs a) {
  __shared__ int pos[kCombineMaxK];
  __shared__ float w[kCombineMaxK];
  const unsigned t = blockIdx.x;
  if (threadIdx.x < kCombineMaxK) {
    const bool live = (int)threadIdx.x < a.k;
    const int p = live ? a.pos[(size_t)t * a.k + threadIdx.x] : -1;
    pos[threadIdx.x] = (unsigned)p < (unsigned)a.M ? p : -1;
    w[threadIdx.x] = live ? a.w[(size_t)t * a.k + threadIdx.x] : 0.0f;
  }
  __syncthreads();
  const unsigned col = 8u * (blockIdx.y * blockDim.x + threadIdx.x);
  if (col >= (unsigned)a.N) return;
  b8 v[kCombineMaxK];
#pragma unroll
  for (int j = 0; j < kCombineMaxK; ++j) {
    if (pos[j] >= 0) v[j] = *(const b8*)(a.y + (size_t)pos[j] * a.N + col);
  }
  float acc[8];
  if (a.residual) {
    const b8 r = *(const b8*)(a.residual + (size_t)t * a.N + col);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (float)r[e];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
  }
#pragma unroll
  for (int j = 0; j < kCombineMaxK; ++j) {
    if (pos[j] >= 0) {
      const float wj = w[j];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(wj, (float)v[j][e], acc[e]);
    }
  }
  b8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (bf16_t)acc[e];
  *(b8*)(a.out + (size_t)t * a.N + col) = o;
}

}  // namespace moe
