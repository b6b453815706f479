// What the one body of the eight bf16 SLIDING-WINDOW packed variable-length prefill kernels over a paged KV cache needs (DESIGN 4.4.9 - 4.4.16,
// 4.4.29). The body itself is flash_attn_prefill_paged_varlen_window_body.inc: a list of statements that each __global__ kernel of
// flash_attn_prefill_paged_varlen_window*.cuh includes once, behind the three declarations that say which kernel it is. An inclusion and not a
// device function template: through a function the same statements compile to another instruction stream -- the D = 128 kernels with sinks ran
// 5 - 34 % slower than before and the D = 256 kernel without a cap spilled 71 VGPRs -- while the inclusion leaves the ten instantiations whose
// source it repeats to the letter byte for byte as they were (DESIGN 4.4.29 has both tables).
// It is the body of fa2b::fa2_prefill_paged_varlen_bf16_mfma (flash_attn_prefill_paged_varlen_bf16.cuh, which has the numerics;
// flash_attn_prefill_paged_varlen.cuh has the slot mapping and the contract) with a window: the query at position
// p = len_b - T_b + t sees the keys max(0, p - W + 1) <= j <= p, W keys, its own among them. What the window changes:
//   key loop     starts at k_begin = align_down(lower edge of the tile's first token, 64), and so does the prefetch; a tile walks at most about
//                W + 128 / G + 2 64 keys whatever len_b is, and reads no table entry and no pool row below k_begin
//   skipped      a wave skips the steps that lie wholly below the lower edge of its own first row, as it skips those past its last row's keys
//   softmax      the select is lo_q <= key < nq, with a per-lane lower edge beside nq
//   fast path    the unmasked step is taken when k0 >= the lower edge of the 16-row tile's LAST row and k0 + 64 <= the keys of its first
// With W >= max_pages page every lower edge is 0 and the arithmetic of a row is the unwindowed kernel's, operation for operation.
//
// What differs between the kernels is resolved at compile time, and nothing else differs:
//   D, CAP   the head dim (64, 128; 256 with the launch bounds and the budget of ..._d256_bf16.cuh) and logit soft-capping. CAP = false: the
//            score multiplier scale_log2 is the caller's x log2(e), log2(e) / sqrt(D) by default. CAP = true: softmax_step_window_cap
//            (paged_softcap.cuh) in place of softmax_step_window -- per score cap2 tanh(q.k x / cap), THEN the mask select: a hidden key is
//            -inf, not -cap -- then the same max / exp2 / row sum. The sink is neither scaled nor capped.
//   GM       the group map, GroupPow2 or GroupAny below: row r of the T G query rows of a (sequence, KV head) is (t, g) = (r / G, r mod G).
//            G touches the prologue (R = T G, Hq = Hkv G, the slot of a sequence, the token of the tile's, the wave's and the 16-row blocks'
//            edge rows), that row map and the epilogue (the output row row_bt + t Hq + g, the sink's head sp.h G + g); never the key loop.
//   SINKS    the sink of query head h, sinks[h] in natural-log units and not scaled by 1/sqrt(D), joins the softmax denominator of every row
//            of that head that sees a key, and carries no value. It is loaded behind the key loop, in the epilogue, where m and l are still
//            fp32 registers, and enters there once (fold_sink). A tile whose rows see no key (n_end <= 0) returns before it with O = 0 and
//            LSE = -inf: the sink does not turn a non-row into a row. kOptional: sinks may be null, the bits of sinks that are all -inf.
//   kv       the pool view (Pool<> below). fa2b::PagedKV: bf16 pools, 16-byte pieces copied to LDS. fa2d::PagedKV8: pools in FP8 (OCP e4m3fn, one fp32
//            scale per KV head, value = code * scale[kv head]) -- a thread keeps the bf16 geometry of the staging stage (the same 8-element
//            column of D / 32 rows of a step) and so loads 8 BYTES per row and tensor; the bytes wait in registers while the step before is
//            computed (half the staging registers) and become bf16 once, on their way into LDS (e4m3x8_to_b8, exact). The LDS image, both
//            products and the softmax run on the unscaled codes. k_scale[h] is part of the dequantised score, so it multiplies what stands
//            inside the tanh: scale_log2 and pre take it once per workgroup, cap2 does not. v_scale[h] multiplies the final 1 / l.
#pragma once
#include <type_traits>

#include "flash_attn_paged_bf16_fp8_rows.cuh"  // e4m3x8_to_b8, sink_log2_or_none; sink_log2 and fold_sink; fa2d::PagedKV8
#include "flash_attn_prefill_paged_varlen_bf16.cuh"
#include "paged_anyg.cuh"  // tok_of
#include "paged_softcap.cuh"

namespace fa2pp {

// The slots for any G: per KV head the grid has total_q G / 128 + B workgroups, and sequence b owns those from s_b = cu_q[b] G / 128 + b. The
// disjointness proof of flash_attn_prefill_paged_varlen.cuh uses only floor((x + y) / 128) >= floor(x / 128) + floor(y / 128) with
// x = cu_q[b] G and y = T_b G, which holds for any integers: s_{b+1} >= s_b + ceil(T_b G / 128) for any G, the ranges are disjoint and every
// tile has a slot.
// fa2pp::slot_of for any G: the first slot of sequence b whose (clamped) first packed row is c; c G < 2^31: the host checked that the grid fits
__device__ __forceinline__ unsigned slot_of_anyg(int c, int G, int b) { return (unsigned)c * (unsigned)G / (unsigned)kRowTile + (unsigned)b; }

// fa2pp::seq_of_slot on slot_of_anyg
__device__ __forceinline__ int seq_of_slot_anyg(const int* __restrict__ cu_q, int B, int total_q, int G, unsigned slot, int& c0, int& T) {
  int lo = 0, hi = B;  // s_b <= slot for every b < lo, s_b > slot for every b >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int c = min(max(cu_q[mid], 0), total_q);
    if (slot_of_anyg(c, G, mid) <= slot)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int b = __builtin_amdgcn_readfirstlane(lo - 1);
  if (b < 0) return -1;
  c0 = __builtin_amdgcn_readfirstlane(min(max(cu_q[b], 0), total_q));
  T = __builtin_amdgcn_readfirstlane(max(min(max(cu_q[b + 1], 0), total_q) - c0, 0));
  return b;
}

}  // namespace fa2pp

namespace fa2b {

using fa2pp::tok_of;

// the first key a query that sees the keys below nq sees under a window of W: max(0, nq - W), without an overflow for nq <= 0 or a W near 2^31
__host__ __device__ __forceinline__ int window_edge(int nq, int W) { return nq > W ? nq - W : 0; }

// fa2b::softmax_step with a lower edge: the keys lo_q <= key < nq of the step are visible
template <bool MASK>
__device__ __forceinline__ void softmax_step_window(const f4 (&st)[kKB], unsigned key0, unsigned lo_q, unsigned nq, float scale_log2, float& m,
                                                    float& l, float& alpha, b8 (&pf)[2]) {
  float sc[4 * kKB];
  float mx = FA2D_NEG_INF;
#pragma unroll
  for (int e = 0; e < 4 * kKB; ++e) {
    const float s = st[e >> 2][e & 3] * scale_log2;
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

// The group maps. `a` is the kernel's group argument: g_shift with G = 2^g_shift = size(a), or G itself in 1 ... 16. The divisions of GroupAny are plain
// unsigned 32-bit divisions, exact for every r < 2^32 and so for every row the host lets through (R = total_q G <= 2^31 - 1).
struct GroupPow2 {
  static __device__ __forceinline__ int size(int a) { return 1 << a; }
  static __device__ __forceinline__ int times(int x, int a) { return x << a; }
  static __device__ __forceinline__ int tok(int r, int a) { return r >> a; }
  static __device__ __forceinline__ int head(int r, int, int G) { return r & (G - 1); }
  static __device__ __forceinline__ unsigned slot_of(int c, int a, int b) { return fa2pp::slot_of(c, a, b); }
  static __device__ __forceinline__ int seq_of_slot(const int* __restrict__ cu_q, int B, int total_q, int a, unsigned slot, int& c0, int& T) {
    return fa2pp::seq_of_slot(cu_q, B, total_q, a, slot, c0, T);
  }
};
struct GroupAny {
  static __device__ __forceinline__ int size(int a) { return a; }
  static __device__ __forceinline__ int times(int x, int a) { return x * a; }
  static __device__ __forceinline__ int tok(int r, int a) { return tok_of(r, a); }
  static __device__ __forceinline__ int head(int r, int t, int G) { return r - t * G; }
  static __device__ __forceinline__ unsigned slot_of(int c, int a, int b) { return fa2pp::slot_of_anyg(c, a, b); }
  static __device__ __forceinline__ int seq_of_slot(const int* __restrict__ cu_q, int B, int total_q, int a, unsigned slot, int& c0, int& T) {
    return fa2pp::seq_of_slot_anyg(cu_q, B, total_q, a, slot, c0, T);
  }
};

enum class Sinks { kNone, kRequired, kOptional };


// The pool views: what a thread stages per row and tensor and how it becomes the bf16 of the LDS image, and the per-head scales of FP8 pools.
template <class KV>
struct Pool;
template <>
struct Pool<PagedKV> {
  static constexpr bool kFp8 = false;
  using Piece = b8;  // 16 bytes, copied
  static __device__ __forceinline__ void clear(b8& x) { x = b8{}; }
  static __device__ __forceinline__ PagedKV::At at(const PagedKV& kv, const fa2d::Split& sp, int D, int col) { return kv.at(sp, D, col); }
  static __device__ __forceinline__ b8 to_b8(b8 x) { return x; }
  static __device__ __forceinline__ float k_scale(const PagedKV&, unsigned) { return 1.0f; }
  static __device__ __forceinline__ float v_scale(const PagedKV&, unsigned) { return 1.0f; }
};
template <>
struct Pool<fa2d::PagedKV8> {
  static constexpr bool kFp8 = true;
  using Piece = uint2;  // 8 bytes of e4m3 codes
  static __device__ __forceinline__ void clear(uint2& x) { x = uint2{0u, 0u}; }
  static __device__ __forceinline__ fa2d::PagedKV8::At at(const fa2d::PagedKV8& kv, const fa2d::Split& sp, int, int col) { return kv.at(sp, col); }
  static __device__ __forceinline__ b8 to_b8(uint2 x) { return e4m3x8_to_b8(x); }
  static __device__ __forceinline__ float k_scale(const fa2d::PagedKV8& kv, unsigned h) { return kv.k_scale[h]; }
  static __device__ __forceinline__ float v_scale(const fa2d::PagedKV8& kv, unsigned h) { return kv.v_scale[h]; }
};

}  // namespace fa2b
