// Logit soft-capping of the *_softcap_* paged attention kernels: the score of a key under a cap, s = cap tanh(q.k x / cap), in
// the log2 units of the online softmax, and the prefill's softmax step on it. Shared by the four kernel headers; nothing else includes it.
//
// gfx950 has no tanh instruction (v_tanh_* came with later ISAs), so tanh is put together in fp32 from v_exp_f32 and v_rcp_f32. With
// y = q.k x / cap and three wave-uniform numbers of paged::softcap_arg -- mult = x log2(e), pre = 2 log2(e) x / cap, cap2 = cap log2(e); the FP8
// kernels multiply mult and pre by k_scale[h] once per workgroup, as it is part of the dequantised score --
//   y^2 >= 2^-10:  cap2 tanh(y) = cap2 - 2 cap2 / (1 + exp2(q.k pre))   one exp, one add, one rcp, one fma. It saturates by itself: exp2 -> inf
//                  gives cap2, exp2 -> 0 gives -cap2, and no finite input gives a NaN. Its error is absolute, about 2^-23 cap2: 1 ulp of
//                  v_rcp_f32 at 1/2 doubled, and the exp's.
//   y^2 <  2^-10:  cap2 tanh(y) = (q.k mult) (1 - y^2 / 3)              relative error 2 y^4 / 15 < 2^-22. Without this branch the absolute error
//                  above would stand beside scores of any size: a cap of 1e30 would turn every score into 0. With it a cap far above the
//                  scores gives the uncapped score q.k mult bit for bit (y^2 underflows, the factor is 1).
// Both are computed and one is selected: no divergence. Per score that is 11 VALU instructions, two of them quarter-rate, where the uncapped
// kernels have one multiplication.
#pragma once
#include "flash_attn_prefill_paged_varlen_window_bf16.cuh"  // softmax_step_window, whose sibling stands below

namespace fa2b {

struct SoftCapMul {
  float mult, pre, cap2;  // wave-uniform
};

__device__ __forceinline__ float softcap_score(float st, const SoftCapMul& c) {
  constexpr float kThird = 0.04003775f;   // 1 / (3 (2 log2 e)^2): y^2 / 3 from (q.k pre)^2
  constexpr float kSmall = 0.008130348f;  // (2 log2 e)^2 2^-10
  const float y2 = st * c.pre, q = y2 * y2;
  const float big = c.cap2 * __builtin_fmaf(__builtin_amdgcn_rcpf(1.0f + fa2d::ex2(y2)), -2.0f, 1.0f);  // one scalar operand per instruction
  const float small = (st * c.mult) * __builtin_fmaf(q, -kThird, 1.0f);
  return q < kSmall ? small : big;
}

// A float kept in an accumulation register between its uses, for the one decode instantiation whose VGPRs are full (PARK; else the identity):
// what the register allocator does by itself when it runs out, written down, so that it is a placement and not a spill.
template <bool PARK>
__device__ __forceinline__ float acc_park(float x) {
  if constexpr (!PARK) return x;
  float a;
  asm("v_accvgpr_write_b32 %0, %1" : "=a"(a) : "v"(x));
  return a;
}
template <bool PARK>
__device__ __forceinline__ float acc_fetch(float a) {
  if constexpr (!PARK) return a;
  float x;
  asm("v_accvgpr_read_b32 %0, %1" : "=v"(x) : "a"(a));
  return x;
}

// fa2b::softmax_step_window with the cap in front of the mask: a hidden key is -inf, not -cap. Behind the scores it is that function, statement
// for statement.
template <bool MASK>
__device__ __forceinline__ void softmax_step_window_cap(const f4 (&st)[kKB], unsigned key0, unsigned lo_q, unsigned nq, const SoftCapMul& cm, float& m,
                                                        float& l, float& alpha, b8 (&pf)[2]) {
  float sc[4 * kKB];
  float mx = FA2D_NEG_INF;
#pragma unroll
  for (int e = 0; e < 4 * kKB; ++e) {
    const float s = softcap_score(st[e >> 2][e & 3], cm);
    const unsigned key = key0 + 16 * (e >> 2) + (e & 3);
    sc[e] = (!MASK || (lo_q <= key && key < nq)) ? s : FA2D_NEG_INF;
    mx = fmaxf(mx, sc[e]);
  }
  float a, c;
  fa2d::swap_pair<16>(mx, a, c);
  mx = fmaxf(a, c);
  fa2d::swap_pair<32>(mx, a, c);
  mx = fmaxf(a, c);  // the maximum over the 64 keys of the step, the same in the four lanes of a query
  const float mn = fmaxf(m, mx);
  const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no visible key yet: every factor below is exp2(-inf) = 0
  alpha = fa2d::ex2(m - ms);
  float ps = 0.0f;
#pragma unroll
  for (int e = 0; e < 4 * kKB; ++e) {
    const float p = fa2d::ex2(sc[e] - ms);
    ps += p;
    pf[e >> 3][e & 7] = (bf16_t)p;
  }
  l = l * alpha + ps;
  m = mn;
}

}  // namespace fa2b
