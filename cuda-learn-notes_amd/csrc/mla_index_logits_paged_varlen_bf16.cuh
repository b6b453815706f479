// The logits of DeepSeek-V3.2's indexer for a PACKED batch with a per-sequence number of query tokens (cln_mla_index_logits_paged_varlen_bf16,
// include/cln_amd_ext.h): mla_index_logits_paged_bf16_mfma (mla_index_logits_paged_bf16.cuh) behind another prologue. q_idx
// bf16 [total_q,Hi,128], weights fp32 [total_q,Hi], logits fp32 [total_q,ld]; cu_q int32 [B + 1] ON THE DEVICE, like the table and the
// lengths. Packed row r is token t = r - cu_q[b] of the sequence b that dsav::packed_row (dsa_varlen_row.cuh) finds, and
//   vis(r) = clamp(seqlens[b], 0, cap) - (T_b - 1 - t),   T_b = cu_q[b + 1] - cu_q[b];
// logits[r, j] is written for 0 <= j < vis(r) and nothing else. A row of no sequence writes nothing and reads no length, table entry or key.
//
// Workgroup blockIdx.x = r chunks + c serves chunk c of packed row r. Everything behind the prologue is the sibling's body, statement for
// statement -- the loaders, the products, the order of the head sum, no LDS, no barrier, __launch_bounds__(256, 2) -- with tok = r: for
// cu_q = [0, T, 2 T, ...] the same bits. IndexKeys and the idx:: numbers are the sibling's (its kernel is a template: including its header
// defines nothing twice).
#pragma once
#include "dsa_varlen_row.cuh"
#include "mla_index_logits_paged_bf16.cuh"

namespace fa2b {

template <int NHB>  // blocks of 16 heads: ceil(Hi / 16)
__global__ __launch_bounds__(kThreads, 2) void mla_index_logits_paged_varlen_bf16_mfma(const bf16_t* __restrict__ q,
                                                                                       const float* __restrict__ weights, const IndexKeys kv,
                                                                                       const int* __restrict__ seqlens,
                                                                                       const int* __restrict__ cu_q, float* __restrict__ logits,
                                                                                       int B, int total_q, int Hi, int cap, int chunks,
                                                                                       long long ld) {
  constexpr int D = idx::kDim, KS = D / 32, KB = idx::kBlocks;
  static_assert(KB == 16, "a lane of the low 16 holds the table entry of one block");
  // the job of workgroup blockIdx.x = r chunks + c, r the packed row
  const unsigned tok = blockIdx.x / (unsigned)chunks, c = blockIdx.x - tok * (unsigned)chunks;
  const dsav::PackedRow pr = dsav::packed_row(cu_q, B, total_q, tok);
  if (pr.b < 0) return;  // a row of no sequence: nothing read, nothing written; workgroup-uniform
  const int b = pr.b;
  const int vis = min(max(seqlens[b], 0), cap) - (pr.T - 1 - pr.t);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wlo = (int)c * idx::kChunk + w * (16 * KB);  // the wave's first key; < cap + 1024: no overflow
  if (wlo >= vis) return;                                // vis <= 0 included; no barrier anywhere: a wave is on its own
  const int nb = min(KB, (vis - wlo + 15) >> 4);         // the wave's blocks with a key below vis
  const int i16 = lane & 15, g4 = lane >> 4;

  b8 qf[NHB][KS];
  float wt[NHB][4];
#pragma unroll
  for (int hb = 0; hb < NHB; ++hb) {
    const int h = 16 * hb + i16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      b8 x = {};
      if (h < Hi) x = *reinterpret_cast<const b8*>(q + ((size_t)tok * Hi + h) * D + 32 * ks + 8 * g4);
      qf[hb][ks] = x;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int he = 16 * hb + 4 * g4 + e;
      wt[hb][e] = he < Hi ? weights[(size_t)tok * Hi + he] : 0.0f;
    }
  }

  const int* bt = kv.table + (size_t)b * kv.max_pages;
  const unsigned pmask = (1u << kv.page_shift) - 1u;
  const int jb = wlo + 16 * i16;                              // block i16 of the wave starts here
  const int pgs = jb < vis ? bt[jb >> kv.page_shift] : 0;     // a block at or past vis has no table entry that is ours to read
  // the 16 bytes of this lane for the four k-steps of block kb; a key at or past vis is not addressed: zeros
  auto load = [&](b8(&d)[KS], int kb) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) d[ks] = b8{};
    const int j = wlo + 16 * kb + i16;
    const int pg = kb < nb ? __builtin_amdgcn_readlane(pgs, kb) : -1;  // kb is wave-uniform
    if (j < vis && (unsigned)pg < (unsigned)kv.P) {  // an entry outside [0, P) is outside the caller's contract: zeros, nothing read out of the pool
      const bf16_t* src = kv.pool + ((((size_t)pg) << kv.page_shift) + ((unsigned)j & pmask)) * D + 8 * g4;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) d[ks] = *reinterpret_cast<const b8*>(src + 32 * ks);
    }
  };

  float* out = logits + (size_t)tok * (size_t)ld;
  b8 cur[KS], nx1[KS], nx2[KS];
  load(cur, 0);
  load(nx1, 1);
  for (int kb = 0; kb < nb; ++kb) {
    load(nx2, kb + 2);
    f4 st[NHB];
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb) {
      st[hb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) st[hb] = mfma(qf[hb][ks], cur[ks], st[hb]);
    }
    float acc = 0.0f;
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(wt[hb][e], fmaxf(st[hb][e], 0.0f), acc);  // spelled out: one order, one rounding per head
    float x, y;
    fa2d::swap_pair<16>(acc, x, y);
    acc = x + y;
    fa2d::swap_pair<32>(acc, x, y);
    acc = x + y;  // the sum over all heads of key i16, the same in its four lanes
    const int j = wlo + 16 * kb + i16;
    if (g4 == 0 && j < vis) out[j] = acc;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) cur[ks] = nx1[ks], nx1[ks] = nx2[ks];
  }
}

// chunks = ceil(cap / 1024) workgroups per packed row (paged::index_logits_varlen_shape). No host read of the offsets, the table or the
// lengths, no allocation.
template <int NHB>
int launch_mla_index_logits_varlen(const void* q, const float* weights, const IndexKeys& kv, const int* seqlens, const int* cu_q, float* logits,
                                   int B, int total_q, int Hi, int cap, int chunks, long long ld, long long wgs, hipStream_t stream) {
  CLN_LAUNCH((mla_index_logits_paged_varlen_bf16_mfma<NHB>), dim3((unsigned)wgs), dim3(kThreads), 0, stream, (const bf16_t*)q, weights, kv,
             seqlens, cu_q, logits, B, total_q, Hi, cap, chunks, ld);
  return cln_check_launch();
}

}  // namespace fa2b
