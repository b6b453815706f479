// The logits of DeepSeek-V3.2's indexer over the FP8 (e4m3fn) index-key cache for a PACKED batch with a per-sequence number of query tokens
// (cln_mla_index_logits_paged_varlen_bf16_fp8, include/cln_amd_ext.h): mla_index_logits_paged_bf16_fp8_mfma
// (mla_index_logits_paged_bf16_fp8.cuh) behind the prologue of mla_index_logits_paged_varlen_bf16.cuh. q_idx bf16 [total_q,Hi,128], weights
// fp32 [total_q,Hi], logits fp32 [total_q,ld]; cu_q int32 [B + 1] on the device. Packed row r is token t = r - cu_q[b] of the sequence b that
// dsav::packed_row (dsa_varlen_row.cuh) finds, vis(r) = clamp(seqlens[b], 0, cap) - (T_b - 1 - t); logits[r, j] is written for
// 0 <= j < vis(r) and nothing else; a row of no sequence writes nothing and reads no length, table entry, key or scale.
//
// Everything behind the prologue is the FP8 sibling's body, statement for statement (the 32 contiguous code bytes of a lane, q_idx's
// fragments indexed to match, the scale once per key after the head sum), with tok = r: for cu_q = [0, T, 2 T, ...] the same bits.
// IndexKeysFp8 and IndexKeyFp8Piece are the sibling's (its kernel is a template: including its header defines nothing twice).
#pragma once
#include "dsa_varlen_row.cuh"
#include "mla_index_logits_paged_bf16_fp8.cuh"

namespace fa2b {

template <int NHB>  // blocks of 16 heads: ceil(Hi / 16)
__global__ __launch_bounds__(kThreads, 2) void mla_index_logits_paged_varlen_bf16_fp8_mfma(const bf16_t* __restrict__ q,
                                                                                           const float* __restrict__ weights,
                                                                                           const IndexKeysFp8 kv, const int* __restrict__ seqlens,
                                                                                           const int* __restrict__ cu_q,
                                                                                           float* __restrict__ logits, int B, int total_q, int Hi,
                                                                                           int cap, int chunks, long long ld) {
  constexpr int D = idx::kDim, KS = D / 32, KB = idx::kBlocks;
  static_assert(KB == 16 && KS == 4, "a lane of the low 16 holds the table entry of one block; a lane's 32 bytes are four k-steps of 8 codes");
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
      if (h < Hi) x = *reinterpret_cast<const b8*>(q + ((size_t)tok * Hi + h) * D + 32 * g4 + 8 * ks);  // the dims of the lane's code bytes
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
  const size_t page_bytes = (size_t)132 << kv.page_shift, scales_at = (size_t)D << kv.page_shift;
  const int jb = wlo + 16 * i16;                              // block i16 of the wave starts here
  const int pgs = jb < vis ? bt[jb >> kv.page_shift] : 0;     // a block at or past vis has no table entry that is ours to read
  // the 32 code bytes of this lane and the scale of its key in block kb; a key at or past vis is not addressed: zeros
  auto load = [&](IndexKeyFp8Piece& d, int kb) {
    d.c0 = make_uint4(0u, 0u, 0u, 0u), d.c1 = make_uint4(0u, 0u, 0u, 0u), d.s = 0.0f;
    const int j = wlo + 16 * kb + i16;
    const int pg = kb < nb ? __builtin_amdgcn_readlane(pgs, kb) : -1;  // kb is wave-uniform
    if (j < vis && (unsigned)pg < (unsigned)kv.P) {  // an entry outside [0, P) is outside the caller's contract: zeros, nothing read out of the pool
      const uint8_t* pagep = kv.pool + (size_t)pg * page_bytes;
      const unsigned r = (unsigned)j & pmask;
      const uint4* src = reinterpret_cast<const uint4*>(pagep + (size_t)r * D + 32 * g4);
      d.c0 = src[0], d.c1 = src[1];
      d.s = *reinterpret_cast<const float*>(pagep + scales_at + 4u * r);
    }
  };

  float* out = logits + (size_t)tok * (size_t)ld;
  IndexKeyFp8Piece cur, nx1, nx2;
  load(cur, 0);
  load(nx1, 1);
  for (int kb = 0; kb < nb; ++kb) {
    load(nx2, kb + 2);
    const b8 kf[KS] = {e4m3x8_to_b8(make_uint2(cur.c0.x, cur.c0.y)), e4m3x8_to_b8(make_uint2(cur.c0.z, cur.c0.w)),
                       e4m3x8_to_b8(make_uint2(cur.c1.x, cur.c1.y)), e4m3x8_to_b8(make_uint2(cur.c1.z, cur.c1.w))};
    f4 st[NHB];
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb) {
      st[hb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) st[hb] = mfma(qf[hb][ks], kf[ks], st[hb]);
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
    if (g4 == 0 && j < vis) out[j] = acc * cur.s;  // the key's scale: once, after the head sum
    cur = nx1, nx1 = nx2;
  }
}

// chunks = ceil(cap / 1024) workgroups per packed row (paged::index_logits_varlen_shape). No host read of the offsets, the table or the
// lengths, no allocation.
template <int NHB>
int launch_mla_index_logits_varlen_fp8(const void* q, const float* weights, const IndexKeysFp8& kv, const int* seqlens, const int* cu_q,
                                       float* logits, int B, int total_q, int Hi, int cap, int chunks, long long ld, long long wgs,
                                       hipStream_t stream) {
  CLN_LAUNCH((mla_index_logits_paged_varlen_bf16_fp8_mfma<NHB>), dim3((unsigned)wgs), dim3(kThreads), 0, stream, (const bf16_t*)q, weights, kv,
             seqlens, cu_q, logits, B, total_q, Hi, cap, chunks, ld);
  return cln_check_launch();
}

}  // namespace fa2b
