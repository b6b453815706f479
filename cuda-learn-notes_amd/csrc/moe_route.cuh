// Top-k routing of a mixture-of-experts layer (cln_moe_route_topk, include/cln_amd_ext.h): logits bf16 or fp32 [T, E] ->
// topk_ids int32 [T, k] and topk_weights fp32 [T, k].
//
//   key_i    = l_i                                   (softmax: the bf16 -> fp32 conversion is exact, selection rounds nothing)
//            = s_i + bias_i, s_i = 1 / (1 + exp(-l_i)) in fp32            (sigmoid; bias null = 0)
//   ids      = the k largest keys, slot 0 the largest, equal keys to the lower index
//   weight_j = scale exp(l_j - l_max) / sum        sum over the selected (renormalize) or over all E experts       (softmax)
//            = scale s_j (/ sum of the selected s when renormalize)                                                (sigmoid)
//
// One wave a token, four tokens a 256-thread workgroup; a lane holds NK = ceil(E / 64) keys in registers (expert 64 i + lane in register
// i, so a row is loaded in NK coalesced pieces). k rounds: every lane's best (key, index) over its registers, then the wave-wide arg-max of
// (key, -index) over four DPP moves and the two v_permlane swaps, after which every lane knows the winner and the lane that holds it retires
// it (register indices are compile-time: no scratch). Lane j keeps winner j. The row max is round 0's key (softmax), the sums are wave_sum
// of the same moves. No LDS, no atomics; every branch is wave-uniform but the stores. Finite logits are the caller's contract: with fewer
// than k finite keys an index may repeat or be >= E (cln_moe_sort drops the latter), nothing is addressed outside the row.
#pragma once
#include "paged_bf16.cuh"

namespace moe {

constexpr int kRouteThreads = 256, kRouteMaxE = 512, kRouteMaxK = 16;
enum { kSoftmax = 0, kSigmoid = 1 };

struct RouteArgs {
  const void* logits;
  const float* bias;  // [E] or null
  int* ids;
  float* weights;
  int T, E, k, scoring, renorm;
  float scale;
};

__device__ __forceinline__ float route_load(const float* p) { return *p; }
__device__ __forceinline__ float route_load(const bf16_t* p) { return (float)*p; }
__device__ __forceinline__ float route_sigmoid(float l) { return 1.0f / (1.0f + __expf(-l)); }

// (key, idx) := the better of itself and the pair DPP-moved from another lane
template <int CTRL>
__device__ __forceinline__ void route_better(float& key, int& idx) {
  const float ok = cln_dpp<CTRL>(key);
  const int oi = cln_dpp_i<CTRL>(idx);
  const bool take = ok > key || (ok == key && oi < idx);
  key = take ? ok : key;
  idx = take ? oi : idx;
}
__device__ __forceinline__ void route_better_of(float& key, int& idx, float k0, int i0, float k1, int i1) {
  const bool take = k1 > k0 || (k1 == k0 && i1 < i0);
  key = take ? k1 : k0;
  idx = take ? i1 : i0;
}

template <typename T, int NK>
__global__ __launch_bounds__(kRouteThreads) void moe_route_topk_wave(const RouteArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (kRouteThreads / 64) + (threadIdx.x >> 6);
  if (t >= a.T) return;  // the whole wave
  const T* row = (const T*)a.logits + (size_t)t * a.E;
  const float ninf = -__builtin_inff();
  float key[NK];
  float all = 0.0f;  // softmax without renormalize: this lane's part of sum exp(l - l_max), from the row again once l_max is known
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const int e = 64 * i + lane;
    key[i] = ninf;
    if (e < a.E) {
      const float l = route_load(row + e);
      key[i] = a.scoring == kSigmoid ? route_sigmoid(l) + (a.bias ? a.bias[e] : 0.0f) : l;
    }
  }
  int my_id = 0;
  float lmax = 0.0f;
  for (int j = 0; j < a.k; ++j) {
    float bk = key[0];
    int bi = lane;
#pragma unroll
    for (int i = 1; i < NK; ++i) {
      if (key[i] > bk) bk = key[i], bi = 64 * i + lane;  // ascending i: an equal key keeps the lower index
    }
    route_better<0xB1>(bk, bi);   // quad_perm [1,0,3,2]
    route_better<0x4E>(bk, bi);   // quad_perm [2,3,0,1]
    route_better<0x141>(bk, bi);  // row_half_mirror
    route_better<0x140>(bk, bi);  // row_mirror
    {
      const auto k16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(bk), __float_as_uint(bk), false, false);
      const auto i16 = __builtin_amdgcn_permlane16_swap((unsigned)bi, (unsigned)bi, false, false);
      route_better_of(bk, bi, __uint_as_float(k16[0]), (int)i16[0], __uint_as_float(k16[1]), (int)i16[1]);
      const auto k32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(bk), __float_as_uint(bk), false, false);
      const auto i32 = __builtin_amdgcn_permlane32_swap((unsigned)bi, (unsigned)bi, false, false);
      route_better_of(bk, bi, __uint_as_float(k32[0]), (int)i32[0], __uint_as_float(k32[1]), (int)i32[1]);
    }
    if (j == 0) lmax = bk;
    if (lane == j) my_id = bi;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      if (bi == 64 * i + lane) key[i] = ninf;  // the winner retires
    }
  }
  // lane j < k: the term of winner j from its logit (the row is in cache; the same operations as above give the same s)
  const bool mine = lane < a.k && (unsigned)my_id < (unsigned)a.E;
  const float l = mine ? route_load(row + my_id) : 0.0f;
  float p = 0.0f;
  if (mine) p = a.scoring == kSigmoid ? route_sigmoid(l) : __expf(l - lmax);
  float sum = 1.0f;
  if (a.renorm) {
    sum = wave_sum(p);
  } else if (a.scoring == kSoftmax) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int e = 64 * i + lane;
      if (e < a.E) all += __expf(route_load(row + e) - lmax);
    }
    sum = wave_sum(all);
  }
  if (lane < a.k) {
    a.ids[(size_t)t * a.k + lane] = my_id;
    a.weights[(size_t)t * a.k + lane] = a.scale * (p / sum);
  }
}

}  // namespace moe
