// The exact top-k of DeepSeek-V3.2's indexer for a PACKED batch with a per-sequence number of query tokens (cln_mla_index_topk_varlen,
// include/cln_amd_ext.h): mla_index_topk_rows (mla_index_topk.cuh) behind another prologue. logits fp32 [total_q,ld], indices
// int32 [total_q,topk]; cu_q int32 [B + 1] ON THE DEVICE, like the lengths. Packed row r is token t = r - cu_q[b] of the sequence b that
// dsav::packed_row (dsa_varlen_row.cuh) finds, and with n = max(vis(r), 0), vis(r) = clamp(seqlens[b], 0, ld) - (T_b - 1 - t), the list of
// row r is the sibling's: dense for n <= topk, else the topk first under (logit descending, position ascending) in ascending position order.
// Every one of the topk slots of every row r < total_q is written; a row of no sequence has n = 0 -- all -1 -- and reads no length and no logit.
//
// One workgroup of 1024 threads per packed row. Everything behind the prologue is the sibling's body, statement for statement -- the map to
// keys, the four histogram passes, the ordered pass, 1288 bytes of LDS -- with tok = r: for cu_q = [0, T, 2 T, ...] the same lists. The
// sibling's helpers are restated: its header defines a kernel that is no template, so two compile units cannot both include it.
#pragma once
#include "dsa_varlen_row.cuh"
#include "kv_append_paged.cuh"  // kva::f4u

namespace idxkv {

constexpr int kThreads = 1024, kWaves = kThreads / CLN_WAVE;
constexpr int kBlock = 4 * kThreads;  // positions of a step of the workgroup: the scan block of the ordered pass
constexpr int kLdsBytes = (256 + 2 + 2 * kWaves * 2) * 4;

// the unsigned order of the keys is the order of the logits (greater key = greater logit)
__device__ __forceinline__ unsigned key_of(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the keys of positions i ... i + 3 of a row of n; a position at or past n is not read (its key is 0, and no caller counts it)
__device__ __forceinline__ void load4(const float* __restrict__ row, unsigned i, unsigned n, unsigned (&k)[4]) {
  if (i + 4 <= n) {
    const kva::f4u x = *reinterpret_cast<const kva::f4u*>(row + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = key_of(x[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = i + j < n ? key_of(row[i + j]) : 0u;
  }
}

__global__ __launch_bounds__(kThreads) void mla_index_topk_varlen_rows(const float* __restrict__ logits, const int* __restrict__ seqlens,
                                                                       const int* __restrict__ cu_q, int* __restrict__ indices, int B,
                                                                       int total_q, long long ld, int topk) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sel[2];
  __shared__ unsigned tot[2][kWaves][2];
  static_assert(sizeof(hist) + sizeof(sel) + sizeof(tot) == kLdsBytes, "the describe text states the bytes");
  const unsigned tok = blockIdx.x;  // the packed row, < total_q
  const dsav::PackedRow pr = dsav::packed_row(cu_q, B, total_q, tok);
  // ld < 2^31 (paged::index_topk_varlen_shape); positions are unsigned from here on: i + kBlock < 2^31 + 2^13 does not wrap.
  // A row of no sequence: n = 0, no length read
  const unsigned n = pr.b < 0 ? 0u : (unsigned)max(min(max(seqlens[pr.b], 0), (int)ld) - (pr.T - 1 - pr.t), 0);
  const float* row = logits + (size_t)tok * (size_t)ld;
  int* out = indices + (size_t)tok * (size_t)topk;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  if (n <= (unsigned)topk) {  // the dense list; workgroup-uniform
    for (unsigned k = tid; k < (unsigned)topk; k += kThreads) out[k] = k < n ? (int)k : -1;
    return;
  }

  // ---- the radix select: the key of the topk-th largest logit and how many of its ties are taken
  unsigned prefix = 0u, himask = 0u, krem = (unsigned)topk;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    unsigned k[4] = {}, kn[4] = {};
    unsigned i = 4u * tid;
    if (i < n) load4(row, i, n, k);
    for (; i < n; i += kBlock) {
      if (i + kBlock < n) load4(row, i + kBlock, n, kn);  // in flight across the adds
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < n && (k[j] & himask) == prefix) atomicAdd(&hist[(k[j] >> shift) & 255u], 1u);
#pragma unroll
      for (int j = 0; j < 4; ++j) k[j] = kn[j];
    }
    __syncthreads();
    if (wv == 0) {  // lane l owns the digits 255 - 4 l ... 252 - 4 l, highest first
      unsigned c[4], s = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = hist[255 - 4 * lane - j], s += c[j];
      unsigned inc = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned v = __shfl_up(inc, d, 64);
        if (lane >= d) inc += v;
      }
      unsigned above = inc - s;  // the keys with this prefix and a digit above this lane's
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (above < krem && krem <= above + c[j]) sel[0] = (unsigned)(255 - 4 * lane - j), sel[1] = krem - above;  // exactly one (lane, j)
        above += c[j];
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    himask |= 255u << shift;
    krem = sel[1];  // 1 <= krem <= the keys equal to the prefix so far
  }

  // ---- the ordered pass: selected = above the threshold, or equal to it with fewer than krem ties before it
  const unsigned long long below = (1ull << lane) - 1ull;  // the lanes in front of this one
  unsigned run_gt = 0u, run_eq = 0u;                       // of the blocks before this one; the same in every thread
  unsigned k[4] = {}, kn[4] = {};
  if (4u * tid < n) load4(row, 4u * tid, n, k);
  for (unsigned base = 0, blk = 0; base < n; base += kBlock, ++blk) {
    const unsigned i = base + 4u * tid;
    if (i + kBlock < n) load4(row, i + kBlock, n, kn);
    bool g[4], e[4];
    unsigned lo_g = 0u, lo_e = 0u, w_g = 0u, w_e = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      g[j] = i + j < n && k[j] > prefix;
      e[j] = i + j < n && k[j] == prefix;
      const unsigned long long mg = __builtin_amdgcn_ballot_w64(g[j]), me = __builtin_amdgcn_ballot_w64(e[j]);
      lo_g += (unsigned)__builtin_popcountll(mg & below), w_g += (unsigned)__builtin_popcountll(mg);
      lo_e += (unsigned)__builtin_popcountll(me & below), w_e += (unsigned)__builtin_popcountll(me);
    }
    if (lane == 0) tot[blk & 1][wv][0] = w_g, tot[blk & 1][wv][1] = w_e;
    __syncthreads();
    unsigned gt = run_gt + lo_g, eq = run_eq + lo_e, all_g = 0u, all_e = 0u;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
      const unsigned a = tot[blk & 1][v][0], c = tot[blk & 1][v][1];
      if (v < wv) gt += a, eq += c;
      all_g += a, all_e += c;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // positions ascend with (thread, j): this thread's earlier positions come first
      const unsigned slot = gt + min(eq, krem);
      if ((g[j] || (e[j] && eq < krem)) && slot < (unsigned)topk) out[slot] = (int)(i + j);
      gt += g[j] ? 1u : 0u, eq += e[j] ? 1u : 0u;
    }
    run_gt += all_g, run_eq += all_e;
    if (run_gt + min(run_eq, krem) >= (unsigned)topk) break;  // the list is full; workgroup-uniform
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = kn[j];
  }
}

inline int launch_mla_index_topk_varlen(const float* logits, const int* seqlens, const int* cu_q, int* indices, int B, int total_q, long long ld,
                                        int topk, hipStream_t stream) {
  CLN_LAUNCH(mla_index_topk_varlen_rows, dim3((unsigned)total_q), dim3(kThreads), 0, stream, logits, seqlens, cu_q, indices, B, total_q, ld, topk);
  return cln_check_launch();
}

}  // namespace idxkv
