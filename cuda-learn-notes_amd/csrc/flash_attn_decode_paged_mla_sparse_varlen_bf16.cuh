// Sparse multi-head latent attention (MLA) decode over a paged latent cache in bf16 for a PACKED batch with a per-sequence number of query
// tokens (cln_fa2_decode_paged_mla_sparse_varlen_bf16, include/cln_amd_ext.h): fa2_decode_paged_mla_sparse_bf16_mfma
// (flash_attn_decode_paged_mla_sparse_bf16.cuh) behind another prologue. q bf16 [total_q,Hq,576], indices int32 [total_q,topk], o bf16
// [total_q,Hq,512], lse fp32 [total_q,Hq]; cu_q int32 [B + 1] ON THE DEVICE, like the table, the lengths and the lists. Packed row r is
// token t = r - cu_q[b] of the sequence b that dsav::packed_row (dsa_varlen_row.cuh) finds; a slot of its list is valid iff
//   0 <= idx < vis(r) = clamp(seqlens[b], 0, max_pages page) - (T_b - 1 - t),   T_b = cu_q[b + 1] - cu_q[b].
//
// Jobs. A workgroup serves one (packed row, group of 64 heads, split of the index list): blockIdx.x = (r HG + hg) S + s. Everything behind
// the prologue is the sibling's body, statement for statement -- the loader's chain index -> table entry -> row, the one LDS image, the 64
// flags in the pads of rows 0 and 1, the online softmax, store_split<512>, every split written -- with tok = r: for cu_q = [0, T, 2 T, ...]
// the same bits.
//
// A row of no sequence has vis = 0 without a length being read: every slot is empty, so no table entry and no pool row is addressed, every
// step is skipped (its q never meets a product) and the row is stored as the sibling stores a token without a valid slot: O = 0,
// LSE = -inf, with splits every partial m = -inf, l = 0, O = 0 -- the combine reads nothing uninitialised.
//
// Registers and LDS: the sibling's (__launch_bounds__(256, 1), 75776 bytes static); the prologue adds scalar registers only.
#pragma once
#include "dsa_varlen_row.cuh"
#include "flash_attn_decode_paged_mla_shared.cuh"  // fa2_decode_combine_bf16_all; paged_bf16.cuh

namespace fa2b {

// The sibling's numbers, restated: its header defines a kernel that is no template, so two compile units cannot both include it. The compile
// unit asserts them against paged_entry.h's.
namespace mlasv {
constexpr int kDc = 512, kDr = 64, kDk = kDc + kDr;  // value dims, rotary dims, key dims of a latent row
constexpr int kKeyStep = 64;                         // index slots per workgroup step: four lanes per row, 16 rows per wave
constexpr int kHeadGroup = kWaves * 16;              // query heads of a token per workgroup
constexpr int kRowBytes = 2 * kDk + 32;              // bytes of a latent row in LDS
constexpr int kLdsBytes = kKeyStep * kRowBytes;
constexpr int kFlagByte = 2 * kDk;                   // the first pad byte of a row: the flags of 32 slots in rows 0 and 1
}  // namespace mlasv

// The pool of latent rows [P, page, 576] behind a block table, and the index lists [total_q, topk] of logical token positions
struct SparseLatentVarlen {
  const bf16_t* pool;
  const int *table, *indices;
  int max_pages, page_shift, topk;
  __host__ __device__ int nmax() const { return max_pages << page_shift; }  // the plan checked that it fits
};

__global__ __launch_bounds__(kThreads, 1) void fa2_decode_paged_mla_sparse_varlen_bf16_mfma(const bf16_t* __restrict__ q,
                                                                                            const SparseLatentVarlen kv,
                                                                                            const int* __restrict__ seqlens,
                                                                                            const int* __restrict__ cu_q, const Out out, int B,
                                                                                            int total_q, int Hq, int HG, int S, int C,
                                                                                            float scale_log2) {
  constexpr int DK = mlasv::kDk, DV = mlasv::kDc;
  constexpr int KS = DK / 32;  // k-steps of S^T: 18
  constexpr int DB = DV / 16;  // 16-dim blocks of O^T: 32
  constexpr int KB = mlasv::kKeyStep / 16;  // 16-key blocks of a step: 4
  constexpr int ROW = mlasv::kRowBytes;
  static_assert(ROW % 64 == 32 && mlasv::kLdsBytes == 75776, "the sibling's image: an odd multiple of 32 bytes; the describe text states the bytes");
  static_assert(mlasv::kFlagByte + 32 == ROW && mlasv::kKeyStep == 64, "64 flag bytes in the pads of rows 0 and 1");
  __shared__ __attribute__((aligned(16))) unsigned char smem[mlasv::kLdsBytes];

  // the job of workgroup blockIdx.x = (r HG + hg) S + s: split s of the index list of packed row r, for the heads 64 hg ... + 63
  const unsigned job = blockIdx.x / (unsigned)S, s = blockIdx.x - job * (unsigned)S;
  const unsigned tok = job / (unsigned)HG, hg = job - tok * (unsigned)HG;  // tok = r < total_q
  const dsav::PackedRow pr = dsav::packed_row(cu_q, B, total_q, tok);
  const unsigned b = (unsigned)max(pr.b, 0);  // a row of no sequence forms the address of table row 0 and never reads it
  // the dense entry's causal edge; a row of no sequence reads no length and has no valid slot
  const int vis = pr.b < 0 ? 0 : min(max(seqlens[b], 0), kv.nmax()) - (pr.T - 1 - pr.t);
  const unsigned uvis = (unsigned)max(vis, 0);                            // valid: (unsigned)idx < uvis, a negative idx is a large unsigned
  const unsigned lo = s * (unsigned)C;                                    // (S - 1) C < topk: no overflow
  const unsigned hi = min(lo + (unsigned)C, (unsigned)kv.topk);           // the slots lo ... hi - 1 are this split's
  const unsigned n = hi - lo;                                             // > 0
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int* bt = kv.table + (size_t)b * kv.max_pages;
  const int* ix = kv.indices + (size_t)tok * kv.topk;
  const unsigned pmask = (1u << kv.page_shift) - 1u;
  const int h = (int)hg * mlasv::kHeadGroup + 16 * w + i16;              // this lane's query head
  const bool active = (int)hg * mlasv::kHeadGroup + 16 * w < Hq;         // wave-uniform: the wave owns a row
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
  unsigned char* fl_st = smem + (row0 >> 5) * ROW + mlasv::kFlagByte + (row0 & 31u);   // the flag byte of slot row0
  const unsigned char* fl_ld = smem + mlasv::kFlagByte + 4 * g4;                        // flags of keys 16 kb + 4 g4 ... + 3: + (kb >> 1) ROW + 16 (kb & 1)
  const unsigned char* k_ld = smem + i16 * ROW + 16 * g4;                              // A of S^T: key row 16 kb + i16, dims 32 ks + 8 g4 ...
  const unsigned char* v_ld = smem + (4 * g4 + (i16 >> 2)) * ROW + 8 * (i16 & 3);      // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m = FA2D_NEG_INF, l = 0.0f;
  f4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  b8 rows[KS];
  int idx = fetch(0), idx2 = fetch(2 * mlasv::kKeyStep);  // idx: of the step whose rows are loaded next; idx2: of the step behind it
  int pg = lookup(idx);
  load(rows, pg, idx);
  bool flag = valid(idx);  // of the rows in flight
  idx = fetch(mlasv::kKeyStep);
  pg = lookup(idx);
  for (unsigned r0 = 0; r0 < n; r0 += mlasv::kKeyStep) {  // n is the workgroup's: every wave takes every barrier
    __syncthreads();  // the reads of the step before are done
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<b8*>(st_p + 64 * ks) = rows[ks];
    if (g4 == 0) *fl_st = flag ? (unsigned char)1 : (unsigned char)0;
    __syncthreads();
    load(rows, pg, idx);  // behind the last step every slot is empty: zeros, no access
    flag = valid(idx);
    pg = lookup(idx2);
    idx = idx2;
    idx2 = fetch(r0 + 3 * mlasv::kKeyStep);
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

// S splits of C index slots (C a multiple of the 64-slot step, S C >= topk > (S - 1) C: paged::mla_sparse_varlen_plan). No host read of the
// offsets, the table, the lengths or the indices, no allocation.
inline int launch_decode_paged_mla_sparse_varlen(const void* q, const SparseLatentVarlen& kv, const int* seqlens, const int* cu_q, void* o,
                                                 float* lse, void* workspace, int B, int total_q, int Hq, int S, int C, float scale_log2,
                                                 hipStream_t stream) {
  const int HG = (Hq + mlasv::kHeadGroup - 1) / mlasv::kHeadGroup;
  const long long rows = (long long)total_q * Hq;
  const Out out = make_out(o, lse, workspace, rows, S, mlasv::kDc);
  CLN_LAUNCH(fa2_decode_paged_mla_sparse_varlen_bf16_mfma, dim3((unsigned)((long long)total_q * HG * S)), dim3(kThreads), 0, stream,
             (const bf16_t*)q, kv, seqlens, cu_q, out, B, total_q, Hq, HG, S, C, scale_log2);
  const int rc = cln_check_launch();
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_combine_bf16_all<mlasv::kDc>), dim3((unsigned)rows), dim3(mlasv::kDc), 0, stream, (const float*)out.ws_o,
             (const float*)out.ws_ml, out.o, out.lse, S);
  return cln_check_launch();
}

}  // namespace fa2b
