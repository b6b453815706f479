// Multi-head latent attention (MLA) decode over a PAGED LATENT cache in bf16 (cln_fa2_decode_paged_mla_bf16, include/cln_amd_ext.h; DESIGN
// 4.4.17): the cache of DeepSeek-V2 / V3 / R1 and Kimi-K2 after the model has absorbed W_UK into q. One pool of latent rows
// [P, page, 576] = [c (512) | k_pe (64)], stored once and shared by every query head: the same row is the KEY (all 576 dims) and the VALUE
// (dims 0 ... 511). q bf16 [B,T,Hq,576], o bf16 [B,T,Hq,512]; row r = t Hq + h of a sequence sees the keys j < len - (T - 1 - t).
//
// Rows over waves. A workgroup of four waves serves one (sequence, split, row group of 64 query rows), each wave one 16-row tile, and every
// wave walks ALL keys of the split: no merge of waves at the end, a wave stores its own rows. Per 64-key step the four waves fetch the 64
// latent rows from global memory ONCE (a lane one row: 18 x 16 bytes, the loads of the next step in flight in 72 registers across the
// products of this one) and put them into ONE LDS image of 64 rows x kMlaRowBytes. That one image feeds both products of every wave:
//   S^T = K Q^T   plain 16-byte row reads as the A operand: 4 key blocks x 18 k-steps = 72 MFMAs, Q fragments (72 registers) as B
//   O^T = V^T P^T transposing reads (ds_read_b64_tr_b16) of dims 0 ... 511 of the same rows: 32 dim blocks x 2 key pairs = 64 MFMAs, all 32
//                 k-slots filled (two 16-key blocks each), P from the S^T registers as B
// The rotary dims (bytes 1024 ... 1151 of a row) are never read by the second product. kMlaRowBytes = 2 x 576 + 32 = 1184 = 37 x 32: an odd
// multiple of 32 bytes, so the 16 rows of a ds_read_b128 lane group and the 8 rows of a 32-lane half of a transposing read fall on distinct
// 32-byte bank groups, as VROW does in the head-dim siblings.
// Registers per wave (the budget, written before the kernel; DESIGN 4.4.17 has the compiled numbers): 128 accumulators (32 dim blocks x 4,
// AGPRs as the MFMAs' C / D operand) + 72 Q + 72 of the next step's rows + 16 scores + 8 P + K / V fragments in flight and addresses: about
// 320, past 256, so __launch_bounds__(256, 1) and the unified file of 512. LDS: one image, 64 x 1184 = 75776 bytes static.
// R <= 16 (Hq = 16, T = 1: 8-way tensor parallel): waves 1 ... 3 own no row; they stage their 16 rows of every step and wait at the barriers.
// Everything behind the loop is the bf16 family's: fa2d::split_of with the row groups in the place of the KV heads, PagedKV with k = v = the
// pool and Hkv = 1 (size_t element arithmetic at a row length of 576), store_split / store_final at D = 512 and, with more than one split,
// fa2_decode_combine_bf16_rows<512>. Rows at or past n of a split are never addressed, nor are their table entries.
#pragma once
#include "paged_bf16.cuh"

namespace fa2b {

constexpr int kMlaDc = 512, kMlaDr = 64, kMlaDk = kMlaDc + kMlaDr;  // value dims, rotary dims, key dims of a latent row
constexpr int kMlaKeyStep = 64;                                    // keys per workgroup step: one row per lane of each of the 4 waves
constexpr int kMlaRowGroup = kWaves * 16;                          // query rows per workgroup
constexpr int kMlaRowBytes = 2 * kMlaDk + 32;                      // bytes of a latent row in LDS
constexpr int kMlaLdsBytes = kMlaKeyStep * kMlaRowBytes;

__global__ __launch_bounds__(kThreads, 1) void fa2_decode_paged_mla_bf16_mfma(const bf16_t* __restrict__ q, const PagedKV kv,
                                                                              const int* __restrict__ seqlens, const Out out, int T, int Hq, int RG,
                                                                              int S, int C, float scale_log2) {
  constexpr int DK = kMlaDk, DV = kMlaDc;
  constexpr int KS = DK / 32;  // k-steps of S^T: 18
  constexpr int DB = DV / 16;  // 16-dim blocks of O^T: 32
  constexpr int KB = kMlaKeyStep / 16;  // 16-key blocks of a step: 4
  constexpr int ROW = kMlaRowBytes;
  static_assert(ROW % 64 == 32 && kMlaLdsBytes == 75776, "an odd multiple of 32 bytes; the describe text states the bytes");
  __shared__ __attribute__((aligned(16))) unsigned char smem[kMlaLdsBytes];

  fa2d::Split sp;
  if (!fa2d::split_of(sp, seqlens, RG, kv.nmax(), S, C)) return;  // "heads" = the row groups of a sequence: sp.h is the row group
  const unsigned n = sp.n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const PagedKV::At at = {kv.k, kv.v, kv.table + (size_t)sp.b * kv.max_pages, 0u, (unsigned)sp.lo, 8 * g4};  // one KV head
  const int R = T * Hq;
  const int r = (int)sp.h * kMlaRowGroup + 16 * w + i16;  // this lane's query row of the sequence, r = t Hq + h
  const bool active = (int)sp.h * kMlaRowGroup + 16 * w < R;  // wave-uniform: the wave owns a row
  const size_t row = (size_t)sp.b * R + r;                // flat row of q, o and lse

  // the query fragments and the keys OF THIS SPLIT the lane's query sees: split-local index < nql (<= 0: none)
  b8 qf[KS];
  const int nql = r < R ? sp.len - (T - 1 - r / Hq) - sp.lo : 0;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    b8 x = {};
    if (r < R) x = *reinterpret_cast<const b8*>(q + row * DK + 32 * ks + 8 * g4);
    qf[ks] = x;
  }

  const unsigned row0 = (unsigned)(16 * w + i16);  // this lane's row of a step
  // a row at or past n is not addressed at all: zeros
  auto load = [&](b8(&d)[KS], int pg, unsigned r0) {
    const unsigned rr = r0 + row0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) d[ks] = b8{};
    if (rr < n) {
      const size_t e = kv.elem(at, pg, rr, DK);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) d[ks] = *reinterpret_cast<const b8*>(at.k + e + 32 * ks);
    }
  };

  unsigned char* st_p = smem + row0 * ROW + 16 * g4;                                  // where this lane puts its 16 bytes of row row0 (+ 64 ks bytes)
  const unsigned char* k_ld = smem + i16 * ROW + 16 * g4;                              // A of S^T: key row 16 kb + i16, dims 32 ks + 8 g4 ...
  const unsigned char* v_ld = smem + (4 * g4 + (i16 >> 2)) * ROW + 8 * (i16 & 3);      // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m = FA2D_NEG_INF, l = 0.0f;
  f4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  b8 rows[KS];
  int pg = kv.lookup(at, row0, n);  // the physical page of this lane's row of the step, fetched one step ahead of the row
  load(rows, pg, 0);
  pg = kv.lookup(at, kMlaKeyStep + row0, n);
  for (unsigned r0 = 0; r0 < n; r0 += kMlaKeyStep) {  // n is the workgroup's: every wave takes every barrier
    __syncthreads();  // the reads of the step before are done
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<b8*>(st_p + 64 * ks) = rows[ks];
    __syncthreads();
    load(rows, pg, r0 + kMlaKeyStep);  // behind the last step the predicate is false: zeros, no access
    pg = kv.lookup(at, r0 + 2 * kMlaKeyStep + row0, n);
    if (active) {
      f4 st[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) st[kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) st[kb] = mfma(*reinterpret_cast<const b8*>(k_ld + 16 * kb * ROW + 64 * ks), qf[ks], st[kb]);
      const int key0 = (int)r0 + 4 * g4;  // split-local index of the key in register 0 of S^T block 0
      float sc[4 * KB];
      float mx = FA2D_NEG_INF;
#pragma unroll
      for (int e = 0; e < 4 * KB; ++e) {
        sc[e] = (key0 + 16 * (e >> 2) + (e & 3) < nql) ? st[e >> 2][e & 3] * scale_log2 : FA2D_NEG_INF;
        mx = fmaxf(mx, sc[e]);
      }
      float a, c;
      fa2d::swap_pair<16>(mx, a, c);
      mx = fmaxf(a, c);
      fa2d::swap_pair<32>(mx, a, c);
      mx = fmaxf(a, c);  // the maximum over the 64 keys of the step, the same in the four lanes of a query
      const float mn = fmaxf(m, mx);
      const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no visible key yet: every factor below is exp2(-inf) = 0
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

  // acc[db][e] is dim 16 db + 4 g4 + e of the lane's row. One split: the finished row; more: the raw partial of split sp.s
  if (r < R) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) store_split<DV>(out, row, 16 * db + 4 * g4 + e, sp.s, S, m, l, acc[db][e]);
  }
}

// S splits of C keys (C a multiple of max(page, the key step), S C >= max_pages page > (S - 1) C: paged::mla_plan). No host read of the table
// or the lengths, no allocation.
inline int launch_decode_paged_mla(const void* q, const PagedKV& kv, const int* seqlens, void* o, float* lse, void* workspace, int B, int T, int Hq,
                                   int S, int C, float scale_log2, hipStream_t stream) {
  const int R = T * Hq, RG = (R + kMlaRowGroup - 1) / kMlaRowGroup;
  const long long rows = (long long)B * R;
  const Out out = make_out(o, lse, workspace, rows, S, kMlaDc);
  CLN_LAUNCH(fa2_decode_paged_mla_bf16_mfma, dim3((unsigned)((long long)B * RG * S)), dim3(kThreads), 0, stream, (const bf16_t*)q, kv, seqlens,
             out, T, Hq, RG, S, C, scale_log2);
  return launch_combine<kMlaDc>(cln_check_launch(), out, seqlens, rows, R, kv.nmax(), S, C, stream);
}

}  // namespace fa2b
