// The scoring half of DeepSeek-V3.2's indexer ("DSA") over a paged index-key cache held in FP8 (OCP e4m3fn) with one fp32 scale per token
// (cln_mla_index_logits_paged_bf16_fp8, include/cln_amd_ext.h): the sibling of mla_index_logits_paged_bf16_mfma
// (mla_index_logits_paged_bf16.cuh) on the pool kv_append_paged_index_bf16_fp8.cuh writes. q_idx stays bf16 [B,T,Hi,128], the weights fp32,
// the logits fp32. With c_j the 128 codes of cache position j read as numbers and s_j its scale,
//   logit[b, t, j] = s_j sum_h w[b, t, h] max(0, q_idx[b, t, h] . c_j)     for 0 <= j < vis(b, t) = clamp(seqlens[b], 0, cap) - (T - 1 - t),
// cap = min(max_pages page, ld). logits[b, t, j] is written for those j and nothing else; no key, scale or table entry at or past vis is read.
//
// The scale is multiplied ONCE PER KEY, AFTER THE HEAD SUM, in fp32. For s_j >= 0 that is the dequantise-then-ReLU form exactly:
// max(0, q . (s c)) = s max(0, q . c). s_j finite and >= 0 is the caller's contract; what the append writes is >= 1e-4 / 448 > 0.
// No NaN code (0x7F, 0xFF) in a visible row is the caller's contract too: the append never writes one for finite keys.
//
// The pool: bytes, a page is 132 page bytes -- codes [page,128] at byte 128 r, then scales [page] fp32 at byte 128 page + 4 r.
//
// Kept from the bf16 kernel, word for word: the job (sequence, query token, chunk of 1024 keys), a wave per 256 keys in 16 blocks of 16, the
// heads on the rows of v_mfma_f32_16x16x32_bf16, the table entries of a wave's 16 blocks as ONE load read back by v_readlane, the keys of block
// kb + 2 in flight across the products of block kb, acc = fma(w, max(s, 0), acc) over hb and e in ascending order and the two permlane swaps,
// padding heads with q = 0 and w = 0 in registers, no LDS and no barrier.
//
// New: the B operand. A lane's share of a key is 32 code bytes, and which 32 dims those are is free -- any fixed permutation of the 128 dims
// applied to both operands leaves every dot product the same sum of the same exact products. Chosen here: lane (i16, g4) takes bytes
// [32 g4, 32 g4 + 32) of ITS key row as TWO dwordx4 loads, so that the four lanes of a key read its 128 bytes as one contiguous run and a key
// costs two load instructions instead of four 8-byte ones (half the VMEM issues of the bf16 loop per key; the 8-byte form would keep the bf16
// kernel's dim order but issue as many loads as it does for half the bytes). K-step ks of the MFMA then multiplies dims 32 g4 + 8 ks ... + 7
// of lane g4, and q's fragment (hb, ks) of that lane is loaded from those same dims (the bf16 kernel: 32 ks + 8 g4). The 8 codes of a k-step
// become bf16 by fa2b::e4m3x8_to_b8 (v_cvt_scalef32_pk_bf16_fp8 at scale 2^0): every e4m3 value is a bf16 value, so the conversion is exact
// and the bf16 x bf16 products stay exact in fp32. s_j is one 4-byte load per key, issued with the key's codes (two blocks ahead). The order
// of operations depends on neither the grid, the batch nor the length; it differs from the bf16 kernel's in which dims an MFMA sums, so the
// two agree bit for bit where the sums are exact and within their bounds elsewhere.
//
// Registers per wave (the budget, written before the kernel; DESIGN 4.4.24 has the compiled numbers): 16 NHB of Q (64 at Hi = 64) + 4 NHB of
// weights (16) + 3 x (8 of codes + 1 scale) (this block and the two in flight: 27, where the bf16 kernel holds 3 x 16; load() zeroes a piece
// in place before it fills it, which takes no register of its own) + 16 of the converted block + 4 NHB accumulators (16) + addresses, about
// 165: __launch_bounds__(256, 2) and 256 registers, two workgroups a CU. LDS: none.
#pragma once
#include "flash_attn_paged_bf16_fp8_rows.cuh"  // e4m3x8_to_b8; paged_bf16.cuh
#include "mla_index_logits_paged_bf16.cuh"     // idx::kDim, kBlocks, kChunk: the job is the bf16 kernel's

namespace fa2b {

// The pool of index keys in FP8 behind the block table: [P, 132 page] bytes
struct IndexKeysFp8 {
  const uint8_t* pool;
  const int* table;
  int P, max_pages, page_shift;
};

// A lane's share of one key in flight: 32 code bytes and the key's scale
struct IndexKeyFp8Piece {
  uint4 c0, c1;
  float s;
};

template <int NHB>  // blocks of 16 heads: ceil(Hi / 16)
__global__ __launch_bounds__(kThreads, 2) void mla_index_logits_paged_bf16_fp8_mfma(const bf16_t* __restrict__ q, const float* __restrict__ weights,
                                                                                    const IndexKeysFp8 kv, const int* __restrict__ seqlens,
                                                                                    float* __restrict__ logits, int T, int Hi, int cap, int chunks,
                                                                                    long long ld) {
  constexpr int D = idx::kDim, KS = D / 32, KB = idx::kBlocks;
  static_assert(KB == 16 && KS == 4, "a lane of the low 16 holds the table entry of one block; a lane's 32 bytes are four k-steps of 8 codes");
  // the job of workgroup blockIdx.x = (b T + t) chunks + c
  const unsigned tok = blockIdx.x / (unsigned)chunks, c = blockIdx.x - tok * (unsigned)chunks;
  const unsigned b = tok / (unsigned)T, t = tok - b * (unsigned)T;
  const int vis = min(max(seqlens[b], 0), cap) - (T - 1 - (int)t);
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

// chunks = ceil(cap / 1024) workgroups per query token (paged::index_logits_shape). No host read of the table or the lengths, no allocation.
template <int NHB>
int launch_mla_index_logits_fp8(const void* q, const float* weights, const IndexKeysFp8& kv, const int* seqlens, float* logits, int T, int Hi,
                                int cap, int chunks, long long ld, long long wgs, hipStream_t stream) {
  CLN_LAUNCH((mla_index_logits_paged_bf16_fp8_mfma<NHB>), dim3((unsigned)wgs), dim3(kThreads), 0, stream, (const bf16_t*)q, weights, kv, seqlens,
             logits, T, Hi, cap, chunks, ld);
  return cln_check_launch();
}

}  // namespace fa2b
