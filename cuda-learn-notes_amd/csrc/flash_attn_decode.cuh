// Single-query ("decode") attention over a KV cache: O[b,h,:] = sum_{j < len_b} softmax_j(q . K_j / sqrt(D)) V_j with q, o fp16 [B,Hq,D] and the
// lengths an int32 [B] array ON THE DEVICE (clamped to [0, Nmax] by the kernels; the host never reads it). One kernel body for two cache forms:
//   DenseKV   K / V caches fp16 [B,H,Nmax,D], one query head per KV head (G = 1): cln_fa2_decode;
//   PagedKV   pools fp16 [P,Hkv,page,D] behind a block table (flash_attn_decode_common.cuh), Hq = G Hkv: cln_fa2_decode_paged
//             (flash_attn_decode_paged.cuh).
//
// One query row leaves the matrix cores nothing to do (2 flops per byte of K and V): the kernel is a stream. A workgroup of 4 waves owns the keys
// [s C, min((s + 1) C, len_b)) of one KV head. A cache row (128 or 256 bytes) is read by D / 8 neighbouring lanes, 16 bytes each, so a wave load covers
// 1 KiB of consecutive rows; a lane holds kRowsPerLane K rows and as many V rows of the current step plus those of the next step in registers
// (2 x 128 bytes per lane in flight, plain global_load_dwordx4: DESIGN 4.3, the "operand streamed once and shared with nobody" case). The workgroup
// serves ALL G query heads of its KV head: every K and V row is loaded once and used G times (G online softmaxes per lane group). Scores are
// fp32 dot products of the fp16 inputs, scaled by log2 e / sqrt(D) IN fp32; the softmax is the online one per lane group (the group of lanes that
// share rows), exp2 of (score - max) with the -inf guard of softmax.hip (no exp2(m - m_new) while m_new is -inf). The partial (m, l, O) of the lane
// groups merge by DPP / permlane swaps inside a wave and through LDS across the four waves, in a fixed order; the splits as
// flash_attn_decode_common.cuh says. No MFMA, no atomics.
#pragma once
#include "flash_attn_decode_common.cuh"

namespace fa2d {

constexpr int kRowsPerLane = 4;  // K rows (and V rows) of one step held by a lane
// keys per workgroup step: 4 waves x 4 loads x (64 lanes / (D / 8) lanes per row) = 128 (D = 64), 64 (D = 128)
constexpr int key_step(int D) { return kWaves * kRowsPerLane * (CLN_WAVE * 8 / D); }

// A dense cache: the rows of a head are consecutive, there is nothing to look up.
struct DenseKV {
  const half_t *k, *v;
  int H, Nmax;
  __host__ __device__ int heads() const { return H; }
  __host__ __device__ int nmax() const { return Nmax; }
  struct At {
    const half_t *k, *v;
  };
  __device__ At at(const Split& w, int D, int off) const {
    const size_t e0 = ((size_t)w.bh * Nmax + w.lo) * D + off;
    return {k + e0, v + e0};
  }
  __device__ int lookup(const At&, unsigned, unsigned) const { return 0; }
  __device__ size_t elem(const At&, int, unsigned r, int D) const { return (size_t)r * D; }
};

template <int D, int G, class KV>
__global__ __launch_bounds__(kThreads) void fa2_decode_kernel(const half_t* __restrict__ q, const KV kv, const int* __restrict__ seqlens,
                                                              const Out out, int S, int C, float scale_log2) {
  static_assert(D == 64 || D == 128, "head dim");
  static_assert(G == 1 || G == 2 || G == 4 || G == 8, "group size");
  constexpr int LPR = D / 8;           // lanes per cache row (16 bytes each)
  constexpr int RPW = CLN_WAVE / LPR;  // rows per wave load
  constexpr int U = kRowsPerLane;
  constexpr unsigned STEP = key_step(D);
  __shared__ float sm_o[G][kWaves][D];
  __shared__ float sm_ml[G][kWaves][2];

  Split w;
  if (!split_of(w, seqlens, kv.heads(), kv.nmax(), S, C)) return;
  const unsigned n = w.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const typename KV::At at = kv.at(w, D, li * 8);
  const size_t head0 = (size_t)w.bh * G;  // b Hq + first query head of the group
  h8 qh[G];
#pragma unroll
  for (int h = 0; h < G; ++h) qh[h] = *reinterpret_cast<const h8*>(q + (head0 + h) * D + li * 8);
  const unsigned row0 = (unsigned)(wave * U * RPW + g);  // this lane's first row of a step; its u-th row is RPW * u further

  struct Rows {
    h8 k[U], v[U];
  };
  auto lookup = [&](int (&pg)[U], unsigned r0) {
#pragma unroll
    for (int u = 0; u < U; ++u) pg[u] = kv.lookup(at, r0 + row0 + u * RPW, n);
  };
  // rows at or past n are not addressed at all (they may lie past the cache, and what lies in the cache past len_b is not ours to read)
  auto load = [&](Rows& d, const int (&pg)[U], unsigned r0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned r = r0 + row0 + u * RPW;
      h8 kk = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r < n) {
        const size_t e = kv.elem(at, pg[u], r, D);
        kk = *reinterpret_cast<const h8*>(at.k + e);
        vv = *reinterpret_cast<const h8*>(at.v + e);
      }
      d.k[u] = kk, d.v[u] = vv;
    }
  };

  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int h = 0; h < G; ++h) {
    m[h] = FA2D_NEG_INF, l[h] = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[h][j] = 0.0f;
  }
  Rows cur;
  int pg[U];
  lookup(pg, 0);
  load(cur, pg, 0);
  lookup(pg, STEP);
  for (unsigned r0 = 0; r0 < n; r0 += STEP) {
    Rows nxt;
    load(nxt, pg, r0 + STEP);  // behind the last step every predicate is false: zeros, no access
    lookup(pg, r0 + 2 * STEP);
#pragma unroll
    for (int h = 0; h < G; ++h) {
      float sc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float d = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf((float)qh[h][j], (float)cur.k[u][j], d);
        d = group_sum<LPR>(d);
        sc[u] = (r0 + row0 + u * RPW < n) ? d * scale_log2 : FA2D_NEG_INF;
      }
      float mn = m[h];
#pragma unroll
      for (int u = 0; u < U; ++u) mn = fmaxf(mn, sc[u]);
      const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no key of this lane group yet: every factor below is exp2(-inf) = 0, never exp2(-inf + inf)
      const float alpha = ex2(m[h] - ms);
      l[h] *= alpha;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[h][j] *= alpha;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = ex2(sc[u] - ms);
        l[h] += p;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] = fmaf(p, (float)cur.v[u][j], acc[h][j]);
      }
      m[h] = mn;
    }
    cur = nxt;
  }

  // per head: the lane groups of a wave (lanes LPR apart hold the same 8 dims), then the four waves through LDS, in a fixed order
#pragma unroll
  for (int h = 0; h < G; ++h) {
    if constexpr (LPR == 8) {
      float po[8];
      const float pm = cln_dpp<0x128>(m[h]), pl = cln_dpp<0x128>(l[h]);  // row_ror:8
#pragma unroll
      for (int j = 0; j < 8; ++j) po[j] = cln_dpp<0x128>(acc[h][j]);
      merge(m[h], l[h], acc[h], pm, pl, po);
    }
    merge_swap<16>(m[h], l[h], acc[h]);
    merge_swap<32>(m[h], l[h], acc[h]);
    if (lane < LPR) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sm_o[h][wave][li * 8 + j] = acc[h][j];
      if (lane == 0) sm_ml[h][wave][0] = m[h], sm_ml[h][wave][1] = l[h];
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < G * D; idx += kThreads) {
    const int h = idx / D, t = idx % D;
    float mx, L, O;
    reduce_waves(&sm_ml[h][0][0], 2, &sm_o[h][0][t], D, mx, L, O);
    store_split<D>(out, head0 + h, t, w.s, S, mx, L, O);
  }
}

// S splits of C keys (C a multiple of the plan's unit, S C >= Nmax > (S - 1) C: the callers check it) of a cache with B heads() KV heads, G query
// heads each. No host read of the lengths or the table, no allocation.
template <int D, int G, class KV>
int launch_decode(const void* q, const KV& kv, const int* seqlens, void* o, float* lse, void* workspace, int B, int S, int C,
                  hipStream_t stream) {
  const long long bk = (long long)B * kv.heads(), rows = bk * G;
  const Out out = make_out(o, lse, workspace, rows, S, D);
  CLN_LAUNCH((fa2_decode_kernel<D, G, KV>), dim3((unsigned)(bk * S)), dim3(kThreads), 0, stream, (const half_t*)q, kv, seqlens, out, S, C,
             scale_log2(D));
  return launch_combine<D>(cln_check_launch(), out, seqlens, rows, kv.heads() * G, kv.nmax(), S, C, stream);
}

}  // namespace fa2d
