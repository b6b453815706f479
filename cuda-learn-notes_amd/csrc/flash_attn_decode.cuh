// Single-query ("decode") attention over a KV cache: O[b,h,:] = sum_{j < len_b} softmax_j(q . K_j / sqrt(D)) V_j with q, o fp16 [B,H,D],
// K / V caches fp16 [B,H,Nmax,D] and the lengths an int32 [B] array ON THE DEVICE (clamped to [0, Nmax] by the kernels; the host never reads it).
//
// One query row leaves the matrix cores nothing to do (2 flops per byte of K and V): the kernel is a stream. A workgroup of 4 waves owns the keys
// [s C, min((s + 1) C, len_b)) of one head. A cache row (128 or 256 bytes) is read by D / 8 neighbouring lanes, 16 bytes each, so a wave load covers
// 1 KiB of consecutive rows; a lane holds kRowsPerLane K rows and as many V rows of the current step plus those of the next step in registers
// (2 x 128 bytes per lane in flight, plain global_load_dwordx4: DESIGN 4.3, the "operand streamed once and shared with nobody" case). Scores are
// fp32 dot products of the fp16 inputs, scaled by log2 e / sqrt(D) IN fp32; the softmax is the online one per lane group (the group of lanes that
// share rows), exp2 of (score - max) with the -inf guard of softmax.hip (no exp2(m - m_new) while m_new is -inf). The partial (m, l, O) of the lane
// groups merge by DPP / permlane swaps inside a wave and through LDS across the four waves, in a fixed order.
//
// With one split the workgroup writes fp16 O (and the natural-log LSE); with S > 1 it writes its unnormalised fp32 O and (m, l) to the caller's
// workspace and fa2_decode_combine_kernel merges the splits of a head in ascending s. A split that lies wholly past len_b writes nothing and the
// combine kernel skips it by the same arithmetic on len_b: no workspace cell is read that this call did not write. No MFMA, no atomics.
//
// Workspace layout (floats): O partials [B H][S][D], then (m, l) pairs [B H][S][2]  ->  B H S (D + 2) 4 bytes.
#pragma once
#include "common.h"
#include <math.h>

namespace fa2d {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * CLN_WAVE;
constexpr int kRowsPerLane = 4;  // K rows (and V rows) of one step held by a lane
// keys per workgroup step: 4 waves x 4 loads x (64 lanes / (D / 8) lanes per row) = 128 (D = 64), 64 (D = 128)
constexpr int key_step(int D) { return kWaves * kRowsPerLane * (CLN_WAVE * 8 / D); }

#define FA2D_NEG_INF (-__builtin_huge_valf())

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// sum over the LPR (8 or 16) neighbouring lanes that share a cache row; every lane of the group gets it
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
  v += cln_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += cln_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += cln_dpp<0x141>(v);  // row_half_mirror
  if constexpr (LPR == 16) v += cln_dpp<0x140>(v);  // row_mirror
  return v;
}

// (m, l, o) <- the softmax partial of the union of two key sets; (-inf, 0, 0) is neutral
__device__ __forceinline__ void merge(float& m, float& l, float (&o)[8], float pm, float pl, const float (&po)[8]) {
  const float mx = fmaxf(m, pm);
  const float ms = mx == FA2D_NEG_INF ? 0.0f : mx;
  const float sa = ex2(m - ms), sb = ex2(pm - ms);
  l = l * sa + pl * sb;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = o[j] * sa + po[j] * sb;
  m = mx;
}

template <int WHICH>  // 16: rows 0|1 and 2|3 of the wave; 32: its two halves
__device__ __forceinline__ void swap_pair(float x, float& a, float& b) {
  if constexpr (WHICH == 16) {
    const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    a = __uint_as_float(s[0]), b = __uint_as_float(s[1]);
  } else {
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    a = __uint_as_float(s[0]), b = __uint_as_float(s[1]);
  }
}
// both partners of a permlane swap step end up with merge(first, second) of the pair, bit for bit
template <int WHICH>
__device__ __forceinline__ void merge_swap(float& m, float& l, float (&o)[8]) {
  float ma, mb, la, lb, oa[8], ob[8];
  swap_pair<WHICH>(m, ma, mb);
  swap_pair<WHICH>(l, la, lb);
#pragma unroll
  for (int j = 0; j < 8; ++j) swap_pair<WHICH>(o[j], oa[j], ob[j]);
  merge(ma, la, oa, mb, lb, ob);
  m = ma, l = la;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = oa[j];
}

template <int D>
__global__ __launch_bounds__(kThreads) void fa2_decode_kernel(const half_t* __restrict__ q, const half_t* __restrict__ kc, const half_t* __restrict__ vc,
                                                              const int* __restrict__ seqlens, half_t* __restrict__ o, float* __restrict__ lse,
                                                              float* __restrict__ ws_o, float* __restrict__ ws_ml, int H, int Nmax, int S, int C,
                                                              float scale_log2) {
  static_assert(D == 64 || D == 128, "head dim");
  constexpr int LPR = D / 8;         // lanes per cache row (16 bytes each)
  constexpr int RPW = CLN_WAVE / LPR;  // rows per wave load
  constexpr int U = kRowsPerLane;
  constexpr unsigned STEP = key_step(D);
  __shared__ float sm_o[kWaves][D];
  __shared__ float sm_ml[kWaves][2];

  const unsigned bh = blockIdx.x / (unsigned)S, s = blockIdx.x - bh * (unsigned)S;
  const int len = min(max(seqlens[bh / (unsigned)H], 0), Nmax);
  const int lo = (int)s * C;  // (S - 1) C < Nmax: no overflow
  if (S > 1 && lo >= len) return;  // a split wholly past the length: the combine kernel skips it by the same arithmetic
  const unsigned n = len > lo ? (unsigned)min(C, len - lo) : 0u;  // keys of this workgroup: rows lo .. lo + n - 1

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const size_t head = ((size_t)bh * Nmax + lo) * D + li * 8;
  const half_t* kb = kc + head;
  const half_t* vb = vc + head;
  float qf[8];
  {
    const h8 qh = *reinterpret_cast<const h8*>(q + (size_t)bh * D + li * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = (float)qh[j];
  }
  const unsigned row0 = (unsigned)(w * U * RPW + g);  // this lane's first row of a step; its u-th row is RPW * u further

  struct Rows {
    h8 k[U], v[U];
  };
  // rows at or past n are not addressed at all (they may lie past the cache, and what lies in the cache past len_b is not ours to read)
  auto load = [&](Rows& b, unsigned r0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned r = r0 + row0 + u * RPW;
      h8 kk = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r < n) {
        kk = *reinterpret_cast<const h8*>(kb + (size_t)r * D);
        vv = *reinterpret_cast<const h8*>(vb + (size_t)r * D);
      }
      b.k[u] = kk, b.v[u] = vv;
    }
  };

  float m = FA2D_NEG_INF, l = 0.0f, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  Rows cur;
  load(cur, 0);
  for (unsigned r0 = 0; r0 < n; r0 += STEP) {
    Rows nxt;
    load(nxt, r0 + STEP);  // behind the last step every predicate is false: zeros, no access
    float sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float d = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d = fmaf(qf[j], (float)cur.k[u][j], d);
      d = group_sum<LPR>(d);
      sc[u] = (r0 + row0 + u * RPW < n) ? d * scale_log2 : FA2D_NEG_INF;
    }
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u) mn = fmaxf(mn, sc[u]);
    const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no key of this lane group yet: every factor below is exp2(-inf) = 0, never exp2(-inf + inf)
    const float alpha = ex2(m - ms);
    l *= alpha;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = ex2(sc[u] - ms);
      l += p;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(p, (float)cur.v[u][j], acc[j]);
    }
    m = mn;
    cur = nxt;
  }

  // the lane groups of a wave: lanes LPR apart hold the same 8 dims
  if constexpr (LPR == 8) {
    float po[8];
    const float pm = cln_dpp<0x128>(m), pl = cln_dpp<0x128>(l);  // row_ror:8
#pragma unroll
    for (int j = 0; j < 8; ++j) po[j] = cln_dpp<0x128>(acc[j]);
    merge(m, l, acc, pm, pl, po);
  }
  merge_swap<16>(m, l, acc);
  merge_swap<32>(m, l, acc);
  if (lane < LPR) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sm_o[w][li * 8 + j] = acc[j];
    if (lane == 0) sm_ml[w][0] = m, sm_ml[w][1] = l;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= D) return;
  float mx = sm_ml[0][0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) mx = fmaxf(mx, sm_ml[i][0]);
  const float ms = mx == FA2D_NEG_INF ? 0.0f : mx;
  float L = 0.0f, O = 0.0f;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const float f = ex2(sm_ml[i][0] - ms);
    L += sm_ml[i][1] * f;
    O += sm_o[i][t] * f;
  }
  if (S == 1) {
    const float inv = L > 0.0f ? 1.0f / L : 0.0f;  // len_b = 0: O = 0, LSE = -inf
    o[(size_t)bh * D + t] = (half_t)(O * inv);
    if (lse && t == 0) lse[bh] = L > 0.0f ? (mx + __builtin_log2f(L)) * 0.6931471805599453f : FA2D_NEG_INF;
  } else {
    const size_t cell = (size_t)bh * S + s;
    ws_o[cell * D + t] = O;
    if (t == 0) ws_ml[cell * 2] = mx, ws_ml[cell * 2 + 1] = L;
  }
}

// One workgroup of D threads per head: the live splits ceil(len_b / C) of the head, merged in ascending s.
template <int D>
__global__ __launch_bounds__(D) void fa2_decode_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                               const int* __restrict__ seqlens, half_t* __restrict__ o, float* __restrict__ lse, int H,
                                                               int Nmax, int S, int C) {
  const unsigned bh = blockIdx.x;
  const int t = threadIdx.x;
  const unsigned len = (unsigned)min(max(seqlens[bh / (unsigned)H], 0), Nmax);
  const int live = (int)((len + (unsigned)C - 1u) / (unsigned)C);  // <= S, as S C >= Nmax
  const float* ml = ws_ml + (size_t)bh * S * 2;
  const float* po = ws_o + (size_t)bh * S * D + t;
  float mx = FA2D_NEG_INF;
  for (int s = 0; s < live; ++s) mx = fmaxf(mx, ml[2 * s]);  // finite when live > 0: a live split holds at least one key
  float L = 0.0f, O = 0.0f;
  for (int s = 0; s < live; ++s) {
    const float f = ex2(ml[2 * s] - mx);
    L += ml[2 * s + 1] * f;
    O += po[(size_t)s * D] * f;
  }
  const float inv = L > 0.0f ? 1.0f / L : 0.0f;
  o[(size_t)bh * D + t] = (half_t)(O * inv);
  if (lse && t == 0) lse[bh] = L > 0.0f ? (mx + __builtin_log2f(L)) * 0.6931471805599453f : FA2D_NEG_INF;
}

inline long long workspace_bytes(int B, int H, int S, int D) { return S > 1 ? (long long)B * H * S * (D + 2) * 4 : 0; }

// the grid of the first kernel is B H S workgroups of 256 threads in x; HIP takes at most 2^32 - 1 threads per grid dimension
inline bool grid_fits(int B, int H, int S) { return (long long)B * H * S * kThreads <= 0xffffffffLL; }

// S splits of C keys (C a multiple of key_step(D), S C >= Nmax > (S - 1) C: the callers check it). No host read of seqlens, no allocation.
template <int D>
int launch_decode(const void* q, const void* k, const void* v, const int* seqlens, void* o, float* lse, void* workspace, int B, int H, int Nmax,
                  int S, int C, hipStream_t stream) {
  const float scale_log2 = (float)(1.4426950408889634 / sqrt((double)D));
  float* ws_o = (float*)workspace;
  float* ws_ml = S > 1 ? ws_o + (size_t)B * H * S * D : nullptr;
  CLN_LAUNCH((fa2_decode_kernel<D>), dim3((unsigned)((long long)B * H * S)), dim3(kThreads), 0, stream, (const half_t*)q, (const half_t*)k,
             (const half_t*)v, seqlens, (half_t*)o, lse, ws_o, ws_ml, H, Nmax, S, C, scale_log2);
  int rc = cln_check_launch();
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_combine_kernel<D>), dim3((unsigned)(B * H)), dim3(D), 0, stream, (const float*)ws_o, (const float*)ws_ml, seqlens,
             (half_t*)o, lse, H, Nmax, S, C);
  return cln_check_launch();
}

}  // namespace fa2d
