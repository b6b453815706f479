// The scoring half of DeepSeek-V3.2's indexer ("DSA") over a paged index-key cache in bf16 (cln_mla_index_logits_paged_bf16,
// include/cln_amd_ext.h). Per cached token one index key of 128 dims, shared by all Hi <= 64 index heads; query token (b, t)
// brings q_idx[b, t, h, 0 ... 127] and one fp32 weight w[b, t, h] per head, and
//   logit[b, t, j] = sum_h w[b, t, h] max(0, q_idx[b, t, h] . k_idx[j])     for 0 <= j < vis(b, t) = clamp(seqlens[b], 0, cap) - (T - 1 - t),
// cap = min(max_pages page, ld). logits[b, t, j] is written for those j and nothing else; a key at or past vis is never loaded, nor is its
// table entry.
//
// Jobs. A workgroup of four waves serves one (sequence, query token, chunk of 1024 keys); a wave serves 256 consecutive keys of the chunk as
// 16 blocks of 16. The grid is sized from cap, the lengths stay on the device; a workgroup whose chunk starts at or past vis returns, a wave
// stops behind its last block below vis. There is no split over heads: no workspace, no combine, every logit written once.
//
// The products. S = Q K^T on v_mfma_f32_16x16x32_bf16 with the HEADS as the rows: A = 16 heads x 32 dims of q_idx (lane (i16, g4): head
// 16 hb + i16, dims 32 ks + 8 g4 ...), B = 32 dims x 16 keys (lane (i16, g4): key i16 of the block, the same dims) -- a lane's 16 bytes of B
// are 16 contiguous bytes of ITS key row, so the keys go from global memory straight into the operand registers: no LDS, no barrier. The
// four lanes g4 of a key read 64 contiguous bytes per k-step. D[e] of lane (i16, g4) is head 16 hb + 4 g4 + e against key i16: the ReLU, the
// weight and the head sum are fp32 in registers, acc = fma(w, max(s, 0), acc) over hb = 0 ... NHB - 1, e = 0 ... 3 in that order, then the
// four lanes of a key add up by two permlane swaps in which both partners add the same pair. The order is fixed: it depends on neither the
// grid, the batch nor the length. Heads past Hi in the last block of 16 have q = 0 and w = 0 in registers (never uninitialised ones): exactly 0.
//
// The loader. The table entries of a wave's 16 blocks are ONE load (lane l & 15: the entry of block l & 15, a block lies inside a page as
// page >= 16) ahead of the loop, read back by v_readlane; the keys of block kb + 2 are in flight across the products of block kb.
//
// Registers per wave (the budget, written before the kernel; DESIGN 4.4.22 has the compiled numbers): 16 NHB of Q (64 at Hi = 64) + 4 NHB of
// weights (16) + 3 x 16 of keys (this block and the two in flight) + 4 NHB accumulators (16) + addresses, about 170:
// __launch_bounds__(256, 2) and 256 registers, two workgroups a CU so that eight waves keep loads in flight. LDS: none.
#pragma once
#include "paged_bf16.cuh"

namespace fa2b {

namespace idx {
constexpr int kDim = 128, kMaxHeads = 64;
constexpr int kBlocks = 16;                      // 16-key blocks of a wave
constexpr int kChunk = kWaves * kBlocks * 16;    // keys of a workgroup: 1024
}  // namespace idx

// The pool of index keys [P, page, 128] behind the block table
struct IndexKeys {
  const bf16_t* pool;
  const int* table;
  int P, max_pages, page_shift;
};

template <int NHB>  // blocks of 16 heads: ceil(Hi / 16)
__global__ __launch_bounds__(kThreads, 2) void mla_index_logits_paged_bf16_mfma(const bf16_t* __restrict__ q, const float* __restrict__ weights,
                                                                                const IndexKeys kv, const int* __restrict__ seqlens,
                                                                                float* __restrict__ logits, int T, int Hi, int cap, int chunks,
                                                                                long long ld) {
  constexpr int D = idx::kDim, KS = D / 32, KB = idx::kBlocks;
  static_assert(KB == 16, "a lane of the low 16 holds the table entry of one block");
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

// chunks = ceil(cap / 1024) workgroups per query token (paged::index_logits_shape). No host read of the table or the lengths, no allocation.
template <int NHB>
int launch_mla_index_logits(const void* q, const float* weights, const IndexKeys& kv, const int* seqlens, float* logits, int T, int Hi, int cap,
                            int chunks, long long ld, long long wgs, hipStream_t stream) {
  CLN_LAUNCH((mla_index_logits_paged_bf16_mfma<NHB>), dim3((unsigned)wgs), dim3(kThreads), 0, stream, (const bf16_t*)q, weights, kv, seqlens,
             logits, T, Hi, cap, chunks, ld);
  return cln_check_launch();
}

}  // namespace fa2b
