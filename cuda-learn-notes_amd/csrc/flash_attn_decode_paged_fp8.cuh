// Single-query ("decode") attention over a PAGED KV cache held in FP8 (OCP e4m3fn, one byte per element) with one fp32 scale per KV head:
//   O[b,h,:] = sum_{j < len_b} softmax_j(q[b,h] . (k8_j k_scale[h / G]) / sqrt(D)) (v8_j v_scale[h / G])
// q, o fp16 [B,Hq,D]; k_pages / v_pages e4m3fn [P,Hkv,page,D]; k_scale / v_scale fp32 [Hkv], block_table int32 [B,max_pages] and seqlens int32 [B]
// ON THE DEVICE (the host reads none of them). A stored byte c of KV head h means e4m3(c) * scale[h]; the scales are finite and > 0 and the live
// bytes are no NaN code (0x7f, 0xff): the caller's contract, like the pointers and the table entries (flash_attn_decode_paged.cuh).
//
// The kernel is the stream of flash_attn_decode.cuh with bytes for halves: a cache row (64 or 128 bytes) is read by D / 8 neighbouring lanes,
// 8 bytes each, so a wave load covers 512 bytes of consecutive rows; a lane holds kRowsPerLane8 = 8 K rows and as many V rows of the current
// step plus those of the next step (2 x 128 bytes per lane in flight, as the fp16 kernel has). 8 bytes become 8 floats through four
// v_cvt_pk_f32_fp8, once per row for all G query heads: a step is worked off in two halves of four rows, so that at most 4 K and 4 V rows stand
// converted in registers. The arithmetic behind the conversion is that of fa2d::fa2_decode_kernel. The scales never enter the loop:
//   scores     q . k8 is summed in fp32 and multiplied by k_scale[kvh] * log2 e / sqrt(D), one fp32 product per workgroup;
//   values     the workgroup's O partial is linear in V, so v_scale[kvh] multiplies it once, in front of store_split.
// With that the split, the workspace, the combine kernel and the end of a workgroup are those of flash_attn_decode_common.cuh, untouched.
// No MFMA, no atomics, deterministic.
//
// The kernel's name does not end in _kernel: tests/decode_kernels.py labels every fa2d::*_kernel symbol of the library by the fp16 describe
// texts.
#pragma once
#include "flash_attn_decode_common.cuh"
#include <stdint.h>

namespace fa2d {

constexpr int kRowsPerLane8 = 8;  // K rows (and V rows) of one step held by a lane
constexpr int kRowsPerHalf8 = 4;  // ... of which this many stand converted to fp32 at a time
// keys per workgroup step: 4 waves x 8 loads x (64 lanes / (D / 8) lanes per row) = 256 (D = 64), 128 (D = 128)
constexpr int key_step_fp8(int D) { return kWaves * kRowsPerLane8 * (CLN_WAVE * 8 / D); }

typedef float f2 __attribute__((ext_vector_type(2)));

// 8 e4m3fn bytes -> 8 floats, exactly (every e4m3 value is an fp32 value)
__device__ __forceinline__ void cvt8(float (&f)[8], uint2 b) {
  const f2 a0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b.x, false), a1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b.x, true);
  const f2 a2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b.y, false), a3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b.y, true);
  f[0] = a0[0], f[1] = a0[1], f[2] = a1[0], f[3] = a1[1], f[4] = a2[0], f[5] = a2[1], f[6] = a3[0], f[7] = a3[1];
}

// fa2d::PagedKV with one byte per element, and the two scale arrays. `off` is the lane's own offset (in bytes) inside a row.
struct PagedKV8 {
  const uint8_t *k, *v;
  const float *k_scale, *v_scale;  // [Hkv]
  const int* table;
  int Hkv, max_pages, page_shift;
  __host__ __device__ int heads() const { return Hkv; }
  __host__ __device__ int nmax() const { return max_pages << page_shift; }  // the plan checked that it fits
  struct At {
    const uint8_t *k, *v;
    const int* bt;
    unsigned kvh, lo;
    int off;
  };
  __device__ At at(const Split& w, int off) const { return {k, v, table + (size_t)w.b * max_pages, w.h, (unsigned)w.lo, off}; }
  // the physical page of row r; rows at or past n have no table entry that is ours to read
  __device__ int lookup(const At& a, unsigned r, unsigned n) const { return r < n ? a.bt[(a.lo + r) >> page_shift] : 0; }
  __device__ size_t elem(const At& a, int pg, unsigned r, int D) const {
    return ((((size_t)pg * Hkv + a.kvh) << page_shift) + ((a.lo + r) & ((1u << page_shift) - 1u))) * D + a.off;
  }
};

template <int D, int G>
__global__ __launch_bounds__(kThreads) void fa2_decode_fp8_stream(const half_t* __restrict__ q, const PagedKV8 kv, const int* __restrict__ seqlens,
                                                                  const Out out, int S, int C, float scale_log2) {
  static_assert(D == 64 || D == 128, "head dim");
  static_assert(G == 1 || G == 2 || G == 4 || G == 8, "group size");
  constexpr int LPR = D / 8;           // lanes per cache row (8 bytes each)
  constexpr int RPW = CLN_WAVE / LPR;  // rows per wave load
  constexpr int U = kRowsPerLane8, UH = kRowsPerHalf8;
  constexpr unsigned STEP = key_step_fp8(D);
  __shared__ float sm_o[G][kWaves][D];
  __shared__ float sm_ml[G][kWaves][2];

  Split w;
  if (!split_of(w, seqlens, kv.heads(), kv.nmax(), S, C)) return;
  const unsigned n = w.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const PagedKV8::At at = kv.at(w, li * 8);
  const size_t head0 = (size_t)w.bh * G;  // b Hq + first query head of the group
  const float k_mul = kv.k_scale[w.h] * scale_log2, v_mul = kv.v_scale[w.h];
  h8 qh[G];
#pragma unroll
  for (int h = 0; h < G; ++h) qh[h] = *reinterpret_cast<const h8*>(q + (head0 + h) * D + li * 8);
  const unsigned row0 = (unsigned)(wave * U * RPW + g);  // this lane's first row of a step; its u-th row is RPW * u further

  struct Rows {
    uint2 k[U], v[U];
  };
  auto lookup = [&](int (&pg)[U], unsigned r0) {
#pragma unroll
    for (int u = 0; u < U; ++u) pg[u] = kv.lookup(at, r0 + row0 + u * RPW, n);
  };
  // rows at or past n are not addressed at all (they may lie past the pool, and what lies in a page past len_b is not ours to read)
  auto load = [&](Rows& d, const int (&pg)[U], unsigned r0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned r = r0 + row0 + u * RPW;
      uint2 kk = {0u, 0u}, vv = {0u, 0u};
      if (r < n) {
        const size_t e = kv.elem(at, pg[u], r, D);
        kk = *reinterpret_cast<const uint2*>(at.k + e);
        vv = *reinterpret_cast<const uint2*>(at.v + e);
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
    for (int half = 0; half < U / UH; ++half) {
      float kf[UH][8], vf[UH][8];
#pragma unroll
      for (int u = 0; u < UH; ++u) cvt8(kf[u], cur.k[half * UH + u]), cvt8(vf[u], cur.v[half * UH + u]);
#pragma unroll
      for (int h = 0; h < G; ++h) {
        float sc[UH];
#pragma unroll
        for (int u = 0; u < UH; ++u) {
          float d = 0.0f;
#pragma unroll
          for (int j = 0; j < 8; ++j) d = fmaf((float)qh[h][j], kf[u][j], d);
          d = group_sum<LPR>(d);
          sc[u] = (r0 + row0 + (half * UH + u) * RPW < n) ? d * k_mul : FA2D_NEG_INF;
        }
        float mn = m[h];
#pragma unroll
        for (int u = 0; u < UH; ++u) mn = fmaxf(mn, sc[u]);
        const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no key of this lane group yet: every factor below is exp2(-inf) = 0, never exp2(-inf + inf)
        const float alpha = ex2(m[h] - ms);
        l[h] *= alpha;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] *= alpha;
#pragma unroll
        for (int u = 0; u < UH; ++u) {
          const float p = ex2(sc[u] - ms);
          l[h] += p;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[h][j] = fmaf(p, vf[u][j], acc[h][j]);
        }
        m[h] = mn;
      }
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
    store_split<D>(out, head0 + h, t, w.s, S, mx, L, O * v_mul);  // the partial is linear in V: the value scale once, here
  }
}

// S splits of C keys (C a multiple of max(page, key_step_fp8(D)), S C >= max_pages page > (S - 1) C: the callers check it)
template <int D, int G>
int launch_decode_fp8(const void* q, const PagedKV8& kv, const int* seqlens, void* o, float* lse, void* workspace, int B, int S, int C,
                      hipStream_t stream) {
  const long long bk = (long long)B * kv.heads(), rows = bk * G;
  const Out out = make_out(o, lse, workspace, rows, S, D);
  CLN_LAUNCH((fa2_decode_fp8_stream<D, G>), dim3((unsigned)(bk * S)), dim3(kThreads), 0, stream, (const half_t*)q, kv, seqlens, out, S, C,
             scale_log2(D));
  return launch_combine<D>(cln_check_launch(), out, seqlens, rows, kv.heads() * G, kv.nmax(), S, C, stream);
}

template <int D>
int launch_decode_paged_fp8(int G, const void* q, const PagedKV8& kv, const int* seqlens, void* o, float* lse, void* workspace, int B, int S, int C,
                            hipStream_t stream) {
  switch (G) {
    case 1: return launch_decode_fp8<D, 1>(q, kv, seqlens, o, lse, workspace, B, S, C, stream);
    case 2: return launch_decode_fp8<D, 2>(q, kv, seqlens, o, lse, workspace, B, S, C, stream);
    case 4: return launch_decode_fp8<D, 4>(q, kv, seqlens, o, lse, workspace, B, S, C, stream);
    default: return launch_decode_fp8<D, 8>(q, kv, seqlens, o, lse, workspace, B, S, C, stream);
  }
}

}  // namespace fa2d
