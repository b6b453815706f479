// Single-query ("decode") attention over a PAGED KV cache with grouped query heads:
//   O[b,h,:] = sum_{j < len_b} softmax_j(q[b,h] . K_j / sqrt(D)) V_j,  key j of sequence b and query head h = row j % page of KV head h / G in the
//   physical page block_table[b, j / page].
// q, o fp16 [B,Hq,D]; k_pages / v_pages fp16 [P,Hkv,page,D]; block_table int32 [B,max_pages] and seqlens int32 [B] ON THE DEVICE (the host reads
// neither). Hq = G Hkv, page a power of two (a run-time shift), the lengths clamped to [0, max_pages page] by the kernels.
//
// The structure is that of flash_attn_decode.cuh, whose device helpers are reused: a workgroup of 4 waves streams the keys
// [s C, min((s + 1) C, len_b)) of one (sequence, KV head) to registers, 16 bytes per lane, D / 8 neighbouring lanes per row -- the rows of one head
// in one page are consecutive in memory, so a wave load still covers 1 KiB of consecutive rows wherever the page is at least that long. What is new:
//   * the workgroup serves ALL G query heads of its KV head: every K and V row is loaded once and used G times (G online softmaxes per lane group);
//   * a lane resolves each logical row to (physical page, offset) through the block table. The table entries of a step are fetched one step before
//     its rows, so the dependent chain table -> row is not on the critical path of the stream. Only entries 0 .. ceil(len_b / page) - 1 of a sequence
//     and only rows < len_b of the pages they name are addressed; the entries must lie in [0, P): that is the caller's contract, like the pointers.
// Scores are fp32 dot products scaled by log2 e / sqrt(D) in fp32, the softmax the online one with the -inf guard, all merges in a fixed order.
// With S > 1 the workgroup writes the unnormalised fp32 partials of its G heads and fa2_decode_paged_combine_kernel merges the live splits of a
// query head in ascending s, skipping dead splits by the same arithmetic on len_b: no workspace cell is read that this call did not write.
//
// Workspace layout (floats): O partials [B Hq][S][D], then (m, l) pairs [B Hq][S][2]  ->  B Hq S (D + 2) 4 bytes.
#pragma once
#include "flash_attn_decode.cuh"

namespace fa2p {

using fa2d::kRowsPerLane;
using fa2d::kThreads;
using fa2d::kWaves;

template <int D, int G>
__global__ __launch_bounds__(kThreads) void fa2_decode_paged_kernel(const half_t* __restrict__ q, const half_t* __restrict__ kp,
                                                                    const half_t* __restrict__ vp, const int* __restrict__ block_table,
                                                                    const int* __restrict__ seqlens, half_t* __restrict__ o, float* __restrict__ lse,
                                                                    float* __restrict__ ws_o, float* __restrict__ ws_ml, int Hkv, int max_pages,
                                                                    int page_shift, int S, int C, float scale_log2) {
  static_assert(D == 64 || D == 128, "head dim");
  static_assert(G == 1 || G == 2 || G == 4 || G == 8, "group size");
  constexpr int LPR = D / 8;           // lanes per cache row (16 bytes each)
  constexpr int RPW = CLN_WAVE / LPR;  // rows per wave load
  constexpr int U = kRowsPerLane;
  constexpr unsigned STEP = fa2d::key_step(D);
  __shared__ float sm_o[G][kWaves][D];
  __shared__ float sm_ml[G][kWaves][2];

  const unsigned bk = blockIdx.x / (unsigned)S, s = blockIdx.x - bk * (unsigned)S;  // bk = b Hkv + KV head
  const unsigned b = bk / (unsigned)Hkv, kvh = bk - b * (unsigned)Hkv;
  const int Nmax = max_pages << page_shift;  // the plan checked that it fits
  const int len = min(max(seqlens[b], 0), Nmax);
  const int lo = (int)s * C;  // (S - 1) C < Nmax: no overflow
  if (S > 1 && lo >= len) return;  // a split wholly past the length: the combine kernel skips it by the same arithmetic
  const unsigned n = len > lo ? (unsigned)min(C, len - lo) : 0u;  // keys of this workgroup: logical rows lo .. lo + n - 1

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const int* bt = block_table + (size_t)b * max_pages;
  const unsigned off_mask = (1u << page_shift) - 1u;
  const size_t head0 = (size_t)bk * G;  // b Hq + first query head of the group
  h8 qh[G];
#pragma unroll
  for (int h = 0; h < G; ++h) qh[h] = *reinterpret_cast<const h8*>(q + (head0 + h) * D + li * 8);
  const unsigned row0 = (unsigned)(w * U * RPW + g);  // this lane's first row of a step; its u-th row is RPW * u further

  struct Rows {
    h8 k[U], v[U];
  };
  // the physical pages of this lane's rows of the step at r0; rows at or past n have no table entry that is ours to read
  auto lookup = [&](int (&pg)[U], unsigned r0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned r = r0 + row0 + u * RPW;
      pg[u] = r < n ? bt[((unsigned)lo + r) >> page_shift] : 0;
    }
  };
  // rows at or past n are not addressed at all
  auto load = [&](Rows& d, const int (&pg)[U], unsigned r0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned r = r0 + row0 + u * RPW;
      h8 kk = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r < n) {
        const size_t e = (((((size_t)pg[u] * Hkv + kvh) << page_shift) + (((unsigned)lo + r) & off_mask)) * D) + li * 8;
        kk = *reinterpret_cast<const h8*>(kp + e);
        vv = *reinterpret_cast<const h8*>(vp + e);
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
        d = fa2d::group_sum<LPR>(d);
        sc[u] = (r0 + row0 + u * RPW < n) ? d * scale_log2 : FA2D_NEG_INF;
      }
      float mn = m[h];
#pragma unroll
      for (int u = 0; u < U; ++u) mn = fmaxf(mn, sc[u]);
      const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no key of this lane group yet: every factor below is exp2(-inf) = 0
      const float alpha = fa2d::ex2(m[h] - ms);
      l[h] *= alpha;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[h][j] *= alpha;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = fa2d::ex2(sc[u] - ms);
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
      fa2d::merge(m[h], l[h], acc[h], pm, pl, po);
    }
    fa2d::merge_swap<16>(m[h], l[h], acc[h]);
    fa2d::merge_swap<32>(m[h], l[h], acc[h]);
    if (lane < LPR) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sm_o[h][w][li * 8 + j] = acc[h][j];
      if (lane == 0) sm_ml[h][w][0] = m[h], sm_ml[h][w][1] = l[h];
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < G * D; idx += kThreads) {
    const int h = idx / D, t = idx % D;
    float mx = sm_ml[h][0][0];
#pragma unroll
    for (int i = 1; i < kWaves; ++i) mx = fmaxf(mx, sm_ml[h][i][0]);
    const float ms = mx == FA2D_NEG_INF ? 0.0f : mx;
    float L = 0.0f, O = 0.0f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
      const float f = fa2d::ex2(sm_ml[h][i][0] - ms);
      L += sm_ml[h][i][1] * f;
      O += sm_o[h][i][t] * f;
    }
    const size_t bh = head0 + h;
    if (S == 1) {
      const float inv = L > 0.0f ? 1.0f / L : 0.0f;  // len_b = 0: O = 0, LSE = -inf
      o[bh * D + t] = (half_t)(O * inv);
      if (lse && t == 0) lse[bh] = L > 0.0f ? (mx + __builtin_log2f(L)) * 0.6931471805599453f : FA2D_NEG_INF;
    } else {
      const size_t cell = bh * S + s;
      ws_o[cell * D + t] = O;
      if (t == 0) ws_ml[cell * 2] = mx, ws_ml[cell * 2 + 1] = L;
    }
  }
}

// One workgroup of D threads per query head: the live splits ceil(len_b / C) of the head, merged in ascending s.
template <int D>
__global__ __launch_bounds__(D) void fa2_decode_paged_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                                     const int* __restrict__ seqlens, half_t* __restrict__ o, float* __restrict__ lse,
                                                                     int Hq, int Nmax, int S, int C) {
  const unsigned bh = blockIdx.x;
  const int t = threadIdx.x;
  const unsigned len = (unsigned)min(max(seqlens[bh / (unsigned)Hq], 0), Nmax);
  const int live = (int)((len + (unsigned)C - 1u) / (unsigned)C);  // <= S, as S C >= Nmax
  const float* ml = ws_ml + (size_t)bh * S * 2;
  const float* po = ws_o + (size_t)bh * S * D + t;
  float mx = FA2D_NEG_INF;
  for (int s = 0; s < live; ++s) mx = fmaxf(mx, ml[2 * s]);  // finite when live > 0: a live split holds at least one key
  float L = 0.0f, O = 0.0f;
  for (int s = 0; s < live; ++s) {
    const float f = fa2d::ex2(ml[2 * s] - mx);
    L += ml[2 * s + 1] * f;
    O += po[(size_t)s * D] * f;
  }
  const float inv = L > 0.0f ? 1.0f / L : 0.0f;
  o[(size_t)bh * D + t] = (half_t)(O * inv);
  if (lse && t == 0) lse[bh] = L > 0.0f ? (mx + __builtin_log2f(L)) * 0.6931471805599453f : FA2D_NEG_INF;
}

inline long long workspace_bytes(int B, int Hq, int S, int D) { return S > 1 ? (long long)B * Hq * S * (D + 2) * 4 : 0; }

// B Hkv S workgroups of 256 threads, then B Hq workgroups of D threads, both in x; HIP takes at most 2^32 - 1 threads per grid dimension
inline bool grid_fits(int B, int Hq, int Hkv, int S, int D) {
  return (long long)B * Hkv * S * kThreads <= 0xffffffffLL && (long long)B * Hq * D <= 0xffffffffLL;
}

// S splits of C keys (C a multiple of max(page, key_step(D)), S C >= max_pages page > (S - 1) C: the callers check it). No host read of the table
// or the lengths, no allocation.
template <int D, int G>
int launch_decode_paged(const void* q, const void* kp, const void* vp, const int* block_table, const int* seqlens, void* o, float* lse,
                        void* workspace, int B, int Hkv, int max_pages, int page_shift, int S, int C, hipStream_t stream) {
  const float scale_log2 = (float)(1.4426950408889634 / sqrt((double)D));
  const int Hq = Hkv * G;
  float* ws_o = (float*)workspace;
  float* ws_ml = S > 1 ? ws_o + (size_t)B * Hq * S * D : nullptr;
  CLN_LAUNCH((fa2_decode_paged_kernel<D, G>), dim3((unsigned)((long long)B * Hkv * S)), dim3(kThreads), 0, stream, (const half_t*)q,
             (const half_t*)kp, (const half_t*)vp, block_table, seqlens, (half_t*)o, lse, ws_o, ws_ml, Hkv, max_pages, page_shift, S, C, scale_log2);
  int rc = cln_check_launch();
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_paged_combine_kernel<D>), dim3((unsigned)(B * Hq)), dim3(D), 0, stream, (const float*)ws_o, (const float*)ws_ml, seqlens,
             (half_t*)o, lse, Hq, max_pages << page_shift, S, C);
  return cln_check_launch();
}

}  // namespace fa2p
