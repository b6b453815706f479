// Sparse multi-head latent attention (MLA) decode over a paged latent cache held in FP8 (OCP e4m3fn) with bf16 queries for a PACKED batch
// with a per-sequence number of query tokens (cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8, include/cln_amd_ext.h):
// fa2_decode_paged_mla_sparse_bf16_fp8_mfma (flash_attn_decode_paged_mla_sparse_bf16_fp8.cuh) behind the prologue of
// flash_attn_decode_paged_mla_sparse_varlen_bf16.cuh. q bf16 [total_q,Hq,576], indices int32 [total_q,topk], o bf16 [total_q,Hq,512], lse
// fp32 [total_q,Hq]; cu_q int32 [B + 1] on the device. Packed row r is token t = r - cu_q[b] of the sequence b that dsav::packed_row
// (dsa_varlen_row.cuh) finds; a slot is valid iff 0 <= idx < vis(r) = clamp(seqlens[b], 0, max_pages page) - (T_b - 1 - t).
//
// A workgroup serves one (packed row, group of 64 heads, split of the index list): blockIdx.x = (r HG + hg) S + s. Everything behind the
// prologue is the FP8 sibling's body, statement for statement (the codes converted on their way to the one bf16 LDS image, kv_scale read once
// per workgroup, the score multiplier (softmax_scale log2 e) kv_scale, store_split_scaled<512>, every split written), with tok = r: for
// cu_q = [0, T, 2 T, ...] the same bits. A row of no sequence has vis = 0 without a length being read: no table entry and no pool row is
// addressed, every step is skipped and the row is stored O = 0, LSE = -inf, with splits every partial empty.
//
// Registers and LDS: the sibling's (__launch_bounds__(256, 1), 75776 bytes static); the prologue adds scalar registers only.
#pragma once
#include "dsa_varlen_row.cuh"
#include "flash_attn_paged_bf16_fp8_rows.cuh"      // e4m3x8_to_b8; paged_bf16.cuh
#include "flash_attn_decode_paged_mla_shared.cuh"  // store_split_scaled, fa2_decode_combine_bf16_all

namespace fa2b {

// The siblings' numbers, restated: their headers define kernels that are no templates, so this compile unit cannot include them. The compile
// unit asserts them against paged_entry.h's.
namespace mlasv8 {
constexpr int kDc = 512, kDr = 64, kDk = kDc + kDr;  // value dims, rotary dims, key dims of a latent row
constexpr int kKeyStep = 64;                         // index slots per workgroup step: four lanes per row, 16 rows per wave
constexpr int kHeadGroup = kWaves * 16;              // query heads of a token per workgroup
constexpr int kRowBytes = 2 * kDk + 32;              // bytes of a latent row in the bf16 LDS image
constexpr int kLdsBytes = kKeyStep * kRowBytes;
constexpr int kFlagByte = 2 * kDk;                   // the first pad byte of a row: the flags of 32 slots in rows 0 and 1
constexpr int kCodeLoads = kDk / 64;                 // 16-byte loads of codes per lane and step: 9
}  // namespace mlasv8

// The pool of codes [P, page, 576] behind a block table, and the index lists [total_q, topk] of logical token positions
struct SparseLatentVarlen8 {
  const unsigned char* pool;
  const int *table, *indices;
  int max_pages, page_shift, topk;
  __host__ __device__ int nmax() const { return max_pages << page_shift; }  // the plan checked that it fits
};

__global__ __launch_bounds__(kThreads, 1) void fa2_decode_paged_mla_sparse_varlen_bf16_fp8_mfma(const bf16_t* __restrict__ q,
                                                                                                const SparseLatentVarlen8 kv,
                                                                                                const int* __restrict__ seqlens,
                                                                                                const int* __restrict__ cu_q,
                                                                                                const float* __restrict__ kv_scale, const Out out,
                                                                                                int B, int total_q, int Hq, int HG, int S, int C,
                                                                                                float scale_log2) {
  constexpr int DK = mlasv8::kDk, DV = mlasv8::kDc;
  constexpr int KS = DK / 32;  // k-steps of S^T: 18
  constexpr int DB = DV / 16;  // 16-dim blocks of O^T: 32
  constexpr int KB = mlasv8::kKeyStep / 16;  // 16-key blocks of a step: 4
  constexpr int NL = mlasv8::kCodeLoads;
  constexpr int ROW = mlasv8::kRowBytes;
  static_assert(ROW % 64 == 32 && mlasv8::kLdsBytes == 75776 && NL * 64 == DK, "the siblings' image; a row of codes is 9 x 4 lanes x 16 bytes");
  static_assert(mlasv8::kFlagByte + 32 == ROW && mlasv8::kKeyStep == 64, "64 flag bytes in the pads of rows 0 and 1");
  static_assert(128 * (NL - 1) + 32 * 3 + 32 == mlasv8::kFlagByte, "the converted row ends where the flags begin");
  __shared__ __attribute__((aligned(16))) unsigned char smem[mlasv8::kLdsBytes];

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
  const int h = (int)hg * mlasv8::kHeadGroup + 16 * w + i16;              // this lane's query head
  const bool active = (int)hg * mlasv8::kHeadGroup + 16 * w < Hq;         // wave-uniform: the wave owns a row
  const size_t row = (size_t)tok * Hq + h;                               // flat row of q, o and lse
  const float kvs = *kv_scale;                                           // once per workgroup: a uniform load
  const float mult = scale_log2 * kvs;                                   // (softmax_scale log2 e) kv_scale

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
  // an empty slot is not addressed at all: zero codes
  auto load = [&](uint4(&d)[NL], int pg, int idx) {
#pragma unroll
    for (int i = 0; i < NL; ++i) d[i] = uint4{0u, 0u, 0u, 0u};
    if (valid(idx)) {
      const unsigned char* src = kv.pool + ((((size_t)pg) << kv.page_shift) + ((unsigned)idx & pmask)) * DK + 16 * g4;
#pragma unroll
      for (int i = 0; i < NL; ++i) d[i] = *reinterpret_cast<const uint4*>(src + 64 * i);
    }
  };

  unsigned char* st_p = smem + row0 * ROW + 32 * g4;                                  // where this lane puts its 32 bytes of row row0 (+ 128 i bytes)
  unsigned char* fl_st = smem + (row0 >> 5) * ROW + mlasv8::kFlagByte + (row0 & 31u);  // the flag byte of slot row0
  const unsigned char* fl_ld = smem + mlasv8::kFlagByte + 4 * g4;                       // flags of keys 16 kb + 4 g4 ... + 3: + (kb >> 1) ROW + 16 (kb & 1)
  const unsigned char* k_ld = smem + i16 * ROW + 16 * g4;                              // A of S^T: key row 16 kb + i16, dims 32 ks + 8 g4 ...
  const unsigned char* v_ld = smem + (4 * g4 + (i16 >> 2)) * ROW + 8 * (i16 & 3);      // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m = FA2D_NEG_INF, l = 0.0f;
  f4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  uint4 rows[NL];
  int idx = fetch(0), idx2 = fetch(2 * mlasv8::kKeyStep);  // idx: of the step whose rows are loaded next; idx2: of the step behind it
  int pg = lookup(idx);
  load(rows, pg, idx);
  bool flag = valid(idx);  // of the rows in flight
  idx = fetch(mlasv8::kKeyStep);
  pg = lookup(idx);
  for (unsigned r0 = 0; r0 < n; r0 += mlasv8::kKeyStep) {  // n is the workgroup's: every wave takes every barrier
    __syncthreads();  // the reads of the step before are done
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      *reinterpret_cast<b8*>(st_p + 128 * i) = e4m3x8_to_b8(make_uint2(rows[i].x, rows[i].y));
      *reinterpret_cast<b8*>(st_p + 128 * i + 16) = e4m3x8_to_b8(make_uint2(rows[i].z, rows[i].w));
    }
    if (g4 == 0) *fl_st = flag ? (unsigned char)1 : (unsigned char)0;
    __syncthreads();
    load(rows, pg, idx);  // behind the last step every slot is empty: zeros, no access
    flag = valid(idx);
    pg = lookup(idx2);
    idx = idx2;
    idx2 = fetch(r0 + 3 * mlasv8::kKeyStep);
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
        sc[e] = ((fl[e >> 2] >> (8 * (e & 3))) & 1u) ? st[e >> 2][e & 3] * mult : FA2D_NEG_INF;
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

  // acc[db][e] is dim 16 db + 4 g4 + e of the lane's row, in units of kv_scale. One split: the finished row; more: the partial of split s, an
  // empty one included (0 kv_scale = 0). The head and the row are formed again from a thread index the compiler cannot trace to the one
  // above (an empty asm): three registers less that live across the loop, which is what keeps the kernel from spilling two values to AGPRs
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int he = (int)hg * mlasv8::kHeadGroup + 16 * (tid >> 6) + (tid & 15), ge = (tid & 63) >> 4;
  const size_t rowe = (size_t)tok * Hq + he;
  if (he < Hq) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) store_split_scaled<DV>(out, rowe, 16 * db + 4 * ge + e, s, S, m, l, acc[db][e], kvs);
  }
}

// launch_decode_paged_mla_sparse_varlen with the pool of codes and its scale: the same grid, the same combine
inline int launch_decode_paged_mla_sparse_varlen_fp8(const void* q, const SparseLatentVarlen8& kv, const int* seqlens, const int* cu_q,
                                                     const float* kv_scale, void* o, float* lse, void* workspace, int B, int total_q, int Hq,
                                                     int S, int C, float scale_log2, hipStream_t stream) {
  const int HG = (Hq + mlasv8::kHeadGroup - 1) / mlasv8::kHeadGroup;
  const long long rows = (long long)total_q * Hq;
  const Out out = make_out(o, lse, workspace, rows, S, mlasv8::kDc);
  CLN_LAUNCH(fa2_decode_paged_mla_sparse_varlen_bf16_fp8_mfma, dim3((unsigned)((long long)total_q * HG * S)), dim3(kThreads), 0, stream,
             (const bf16_t*)q, kv, seqlens, cu_q, kv_scale, out, B, total_q, Hq, HG, S, C, scale_log2);
  const int rc = cln_check_launch();
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_combine_bf16_all<mlasv8::kDc>), dim3((unsigned)rows), dim3(mlasv8::kDc), 0, stream, (const float*)out.ws_o,
             (const float*)out.ws_ml, out.o, out.lse, S);
  return cln_check_launch();
}

}  // namespace fa2b
