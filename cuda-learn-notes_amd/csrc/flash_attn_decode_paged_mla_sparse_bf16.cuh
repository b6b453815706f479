// Sparse multi-head latent attention (MLA) decode over a paged latent cache in bf16 (cln_fa2_decode_paged_mla_sparse_bf16,
// include/cln_amd_ext.h): DeepSeek-V3.2's attention ("DSA") behind its indexer. The cache row [c (512) | k_pe (64)] and the
// absorbed query are those of fa2_decode_paged_mla_bf16_mfma (flash_attn_decode_paged_mla_bf16.cuh), whose layout this sibling keeps -- four
// waves, the 64-key step, the ONE LDS image of 64 rows x 1184 bytes that feeds both products, the online softmax, store_split<512>. What
// changes is WHICH rows are keys: query token (b, t) attends only to the cache positions its list indices[b, t, 0 ... topk - 1] names, the
// same list for all its heads. A slot is valid iff 0 <= idx < vis(b, t) = clamp(seqlens[b], 0, max_pages page) - (T - 1 - t); every other
// value is an empty slot, anywhere in the list, and addresses neither a table entry nor a pool row.
//
// Jobs. A workgroup serves one (sequence, query token, group of 64 heads, split of the index list): rows of different tokens have different
// key sets and cannot share a workgroup, so T has no cap. The splits divide the topk SLOTS, not the context (paged::mla_sparse_plan).
//
// The loader. The slot of a lane in a step is lo + r0 + 16 w + i16 (four lanes a row, 18 x 16 bytes each, as in the sibling); a slot at or
// past topk reads no index and counts as -1. The dependent chain is index -> table entry -> row, one link longer than the sibling's, so the
// index is fetched one step ahead of the table entry and that one step ahead of the row: the row loads of the next step are in flight across
// the products of this one. An empty slot loads nothing and its LDS row is zeros (0 x garbage in the second product would be NaN).
//
// The mask. Validity belongs to the key slot and is the same for all 64 query rows; the loader lanes know it, the lanes of the S^T layout
// need it. It travels through LDS in bytes no product reads: every row of the image has 32 pad bytes (1152 ... 1183), and the 64 flags of a
// step are 64 bytes in the pads of rows 0 and 1, flag of key k at byte k & 31 of the pad of row k >> 5, written with the rows between the two
// barriers of a step. A lane's four keys of a 16-key block are then ONE ds_read_b32: four flag reads per step against 200 operand reads, no
// LDS beyond the image, no barrier beyond the sibling's two. (A 64-bit mask from wave ballots would still have to cross the waves through
// LDS.) A step none of whose 64 slots is valid skips both products: with every score -inf they would change no bit.
//
// All S splits of a row are always written -- an empty one as m = -inf, l = 0, O = 0 -- and no workgroup returns early on the lengths: which
// splits are live is not a function of seqlens here. fa2_decode_combine_bf16_all<512> (flash_attn_decode_paged_mla_shared.cuh) merges all S partials in ascending order with the
// family's -inf guard.
//
// Registers per wave (the budget, written before the kernel; DESIGN 4.4.20 has the compiled numbers): the sibling's about 320 (128
// accumulators + 72 Q + 72 of the next step's rows + scores, P, fragments, addresses) + two indices, a page and a flag in flight + four flag
// words: __launch_bounds__(256, 1) and the unified file of 512. LDS: the sibling's one image, 64 x 1184 = 75776 bytes static.
#pragma once
#include "flash_attn_decode_paged_mla_shared.cuh"  // fa2_decode_combine_bf16_all; paged_bf16.cuh

namespace fa2b {

// The sibling's numbers, restated: its header defines a kernel that is no template, so two compile units cannot both include it. The compile
// unit asserts them against paged_entry.h's.
namespace mlas {
constexpr int kDc = 512, kDr = 64, kDk = kDc + kDr;  // value dims, rotary dims, key dims of a latent row
constexpr int kKeyStep = 64;                         // index slots per workgroup step: four lanes per row, 16 rows per wave
constexpr int kHeadGroup = kWaves * 16;              // query heads of a token per workgroup
constexpr int kRowBytes = 2 * kDk + 32;              // bytes of a latent row in LDS
constexpr int kLdsBytes = kKeyStep * kRowBytes;
constexpr int kFlagByte = 2 * kDk;                   // the first pad byte of a row: the flags of 32 slots in rows 0 and 1
}  // namespace mlas

// The pool of latent rows [P, page, 576] behind a block table, and the index lists [B, T, topk] of logical token positions
struct SparseLatent {
  const bf16_t* pool;
  const int *table, *indices;
  int max_pages, page_shift, topk;
  __host__ __device__ int nmax() const { return max_pages << page_shift; }  // the plan checked that it fits
};

__global__ __launch_bounds__(kThreads, 1) void fa2_decode_paged_mla_sparse_bf16_mfma(const bf16_t* __restrict__ q, const SparseLatent kv,
                                                                                     const int* __restrict__ seqlens, const Out out, int T,
                                                                                     int Hq, int HG, int S, int C, float scale_log2) {
  constexpr int DK = mlas::kDk, DV = mlas::kDc;
  constexpr int KS = DK / 32;  // k-steps of S^T: 18
  constexpr int DB = DV / 16;  // 16-dim blocks of O^T: 32
  constexpr int KB = mlas::kKeyStep / 16;  // 16-key blocks of a step: 4
  constexpr int ROW = mlas::kRowBytes;
  static_assert(ROW % 64 == 32 && mlas::kLdsBytes == 75776, "the sibling's image: an odd multiple of 32 bytes; the describe text states the bytes");
  static_assert(mlas::kFlagByte + 32 == ROW && mlas::kKeyStep == 64, "64 flag bytes in the pads of rows 0 and 1");
  __shared__ __attribute__((aligned(16))) unsigned char smem[mlas::kLdsBytes];

  // the job of workgroup blockIdx.x = (((b T + t) HG + hg) S + s: split s of the index list of token (b, t), for the heads 64 hg ... + 63
  const unsigned job = blockIdx.x / (unsigned)S, s = blockIdx.x - job * (unsigned)S;
  const unsigned tok = job / (unsigned)HG, hg = job - tok * (unsigned)HG;  // tok = b T + t
  const unsigned b = tok / (unsigned)T, t = tok - b * (unsigned)T;
  const int vis = min(max(seqlens[b], 0), kv.nmax()) - (T - 1 - (int)t);  // the dense entry's causal edge
  const unsigned uvis = (unsigned)max(vis, 0);                            // valid: (unsigned)idx < uvis, a negative idx is a large unsigned
  const unsigned lo = s * (unsigned)C;                                    // (S - 1) C < topk: no overflow
  const unsigned hi = min(lo + (unsigned)C, (unsigned)kv.topk);           // the slots lo ... hi - 1 are this split's
  const unsigned n = hi - lo;                                             // > 0
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int* bt = kv.table + (size_t)b * kv.max_pages;
  const int* ix = kv.indices + (size_t)tok * kv.topk;
  const unsigned pmask = (1u << kv.page_shift) - 1u;
  const int h = (int)hg * mlas::kHeadGroup + 16 * w + i16;              // this lane's query head
  const bool active = (int)hg * mlas::kHeadGroup + 16 * w < Hq;         // wave-uniform: the wave owns a row
  const size_t row = (size_t)tok * Hq + h;                              // flat row of q, o and lse

  b8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    b8 x = {};
    if (h < Hq) x = *reinterpret_cast<const b8*>(q + row * DK + 32 * ks + 8 * g4);
    qf[ks] = x;
  }

  const unsigned row0 = (unsigned)(16 * w + i16);  // this lane's row of a step
  // the index in this lane's slot of the step at r0; a slot at or past the split's end (or topk) holds no index that is ours to read
  auto fetch = [&](unsigned r0) {
    const unsigned slot = lo + r0 + row0;
    return slot < hi ? ix[slot] : -1;
  };
  auto valid = [&](int idx) { return (unsigned)idx < uvis; };  // uvis <= max_pages page: a valid idx has a table entry
  auto lookup = [&](int idx) { return valid(idx) ? bt[idx >> kv.page_shift] : 0; };
  // an empty slot is not addressed at all: zeros
  auto load = [&](b8(&d)[KS], int pg, int idx) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) d[ks] = b8{};
    if (valid(idx)) {
      const bf16_t* src = kv.pool + ((((size_t)pg) << kv.page_shift) + ((unsigned)idx & pmask)) * DK + 8 * g4;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) d[ks] = *reinterpret_cast<const b8*>(src + 32 * ks);
    }
  };

  unsigned char* st_p = smem + row0 * ROW + 16 * g4;                                  // where this lane puts its 16 bytes of row row0 (+ 64 ks bytes)
  unsigned char* fl_st = smem + (row0 >> 5) * ROW + mlas::kFlagByte + (row0 & 31u);   // the flag byte of slot row0
  const unsigned char* fl_ld = smem + mlas::kFlagByte + 4 * g4;                        // flags of keys 16 kb + 4 g4 ... + 3: + (kb >> 1) ROW + 16 (kb & 1)
  const unsigned char* k_ld = smem + i16 * ROW + 16 * g4;                              // A of S^T: key row 16 kb + i16, dims 32 ks + 8 g4 ...
  const unsigned char* v_ld = smem + (4 * g4 + (i16 >> 2)) * ROW + 8 * (i16 & 3);      // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m = FA2D_NEG_INF, l = 0.0f;
  f4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  b8 rows[KS];
  int idx = fetch(0), idx2 = fetch(2 * mlas::kKeyStep);  // idx: of the step whose rows are loaded next; idx2: of the step behind it
  int pg = lookup(idx);
  load(rows, pg, idx);
  bool flag = valid(idx);  // of the rows in flight
  idx = fetch(mlas::kKeyStep);
  pg = lookup(idx);
  for (unsigned r0 = 0; r0 < n; r0 += mlas::kKeyStep) {  // n is the workgroup's: every wave takes every barrier
    __syncthreads();  // the reads of the step before are done
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<b8*>(st_p + 64 * ks) = rows[ks];
    if (g4 == 0) *fl_st = flag ? (unsigned char)1 : (unsigned char)0;
    __syncthreads();
    load(rows, pg, idx);  // behind the last step every slot is empty: zeros, no access
    flag = valid(idx);
    pg = lookup(idx2);
    idx = idx2;
    idx2 = fetch(r0 + 3 * mlas::kKeyStep);
    if (active) {
      unsigned fl[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) fl[kb] = *reinterpret_cast<const unsigned*>(fl_ld + (kb >> 1) * ROW + 16 * (kb & 1));
      // the four lane groups of a wave hold the flags of all 64 slots between them: wave-uniform
      if (__builtin_amdgcn_ballot_w64((fl[0] | fl[1] | fl[2] | fl[3]) != 0u) == 0ull) continue;
      f4 st[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) st[kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) st[kb] = mfma(*reinterpret_cast<const b8*>(k_ld + 16 * kb * ROW + 64 * ks), qf[ks], st[kb]);
      float sc[4 * KB];
      float mx = FA2D_NEG_INF;
#pragma unroll
      for (int e = 0; e < 4 * KB; ++e) {  // register e & 3 of S^T block e >> 2 is key 16 (e >> 2) + 4 g4 + (e & 3) of the step
        sc[e] = ((fl[e >> 2] >> (8 * (e & 3))) & 1u) ? st[e >> 2][e & 3] * scale_log2 : FA2D_NEG_INF;
        mx = fmaxf(mx, sc[e]);
      }
      float a, c;
      fa2d::swap_pair<16>(mx, a, c);
      mx = fmaxf(a, c);
      fa2d::swap_pair<32>(mx, a, c);
      mx = fmaxf(a, c);  // the maximum over the 64 keys of the step, the same in the four lanes of a query
      const float mn = fmaxf(m, mx);
      const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no valid key yet: every factor below is exp2(-inf) = 0
      const float alpha = fa2d::ex2(m - ms);
      float ps = 0.0f;
      b8 pf[KB / 2];  // k-slots 0 .. 3: key block 2 kp, 4 .. 7: key block 2 kp + 1
#pragma unroll
      for (int e = 0; e < 4 * KB; ++e) {
        const float p = fa2d::ex2(sc[e] - ms);
        ps += p;
        pf[e >> 3][e & 7] = (bf16_t)p;
      }
      l = l * alpha + ps;
      m = mn;
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        acc[db] *= alpha;
#pragma unroll
        for (int kp = 0; kp < KB / 2; ++kp) {
          const b8 vf = b8_cat(lds_read_tr(v_ld + 32 * kp * ROW + 32 * db), lds_read_tr(v_ld + (32 * kp + 16) * ROW + 32 * db));
          acc[db] = mfma(vf, pf[kp], acc[db]);
        }
      }
    }
  }
  if (!active) return;

  // the row sum of the four lanes of a query, in a fixed order (both partners of a swap add the same pair)
  float a, c;
  fa2d::swap_pair<16>(l, a, c);
  l = a + c;
  fa2d::swap_pair<32>(l, a, c);
  l = a + c;

  // acc[db][e] is dim 16 db + 4 g4 + e of the lane's row. One split: the finished row; more: the raw partial of split s, an empty one included
  if (h < Hq) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) store_split<DV>(out, row, 16 * db + 4 * g4 + e, s, S, m, l, acc[db][e]);
  }
}

// S splits of C index slots (C a multiple of the 64-slot step, S C >= topk > (S - 1) C: paged::mla_sparse_plan). No host read of the table,
// the lengths or the indices, no allocation.
inline int launch_decode_paged_mla_sparse(const void* q, const SparseLatent& kv, const int* seqlens, void* o, float* lse, void* workspace, int B,
                                          int T, int Hq, int S, int C, float scale_log2, hipStream_t stream) {
  const int HG = (Hq + mlas::kHeadGroup - 1) / mlas::kHeadGroup;
  const long long rows = (long long)B * T * Hq;
  const Out out = make_out(o, lse, workspace, rows, S, mlas::kDc);
  CLN_LAUNCH(fa2_decode_paged_mla_sparse_bf16_mfma, dim3((unsigned)((long long)B * T * HG * S)), dim3(kThreads), 0, stream, (const bf16_t*)q, kv,
             seqlens, out, T, Hq, HG, S, C, scale_log2);
  const int rc = cln_check_launch();
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_combine_bf16_all<mlas::kDc>), dim3((unsigned)rows), dim3(mlas::kDc), 0, stream, (const float*)out.ws_o,
             (const float*)out.ws_ml, out.o, out.lse, S);
  return cln_check_launch();
}

}  // namespace fa2b
