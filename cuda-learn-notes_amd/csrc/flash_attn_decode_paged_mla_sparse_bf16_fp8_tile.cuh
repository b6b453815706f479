// Sparse multi-head latent attention (MLA) decode over a paged latent cache in DeepSeek-V3.2's OWN FP8 row of 656 bytes, with bf16 queries
// (cln_fa2_decode_paged_mla_sparse_bf16_fp8_tile and cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile, include/cln_amd_ext.h; DESIGN
// 4.4.26). A sibling of fa2_decode_paged_mla_sparse_bf16_fp8_mfma (flash_attn_decode_paged_mla_sparse_bf16_fp8.cuh): the job decomposition,
// the chain index -> table entry -> row with the index two steps and the table entry one step ahead of the row, the 64 validity flags in the
// pad bytes of LDS rows 0 and 1, the ballot skip, the ONE bf16 image of 64 rows x 1184 bytes, both MFMA products read from it exactly as
// fa2_decode_paged_mla_sparse_bf16_mfma reads them, every split written and fa2_decode_combine_bf16_all<512> are that kernel's. What is new
// is WHAT a row is and how it is staged.
//
// The row, 656 bytes a token (the layout FlashMLA's FP8 sparse kernels read):
//   bytes   0 ... 511   512 e4m3fn codes of the latent c
//   bytes 512 ... 527   4 fp32 scales, one per 128-dim tile of c, for this token
//   bytes 528 ... 655   64 bf16 values of k_pe, rotated, not quantised
// and a stored token means c[d] = bf16_rn(fp32(e4m3(code[d])) * scale[d / 128]) -- ONE IEEE fp32 product, ONE rounding to nearest even --
// and k_pe[j] = the stored bf16. No NaN code and finite positive scales in a LISTED row are the caller's contract; an unlisted row is never
// read.
//
// The row fetch. Four lanes share a row. For the next step a lane keeps in flight 8 x 16 bytes of codes (byte 64 i + 16 g4 of the row, all
// inside tile i >> 1), the 16 bytes of scales (one load, the same for the four lanes) and 2 x 16 bytes of k_pe (byte 528 + 64 j + 16 g4):
// 11 loads, 44 registers against the sibling's 36. The row address is ((pg << page_shift) + (idx & pmask)) * 656 BYTES, formed in size_t.
//
// The staging, one path whatever the scale is (v_cvt_scalef32_pk_bf16_fp8 with a scale operand would use the exponent only, so it cannot
// serve): the 16 codes of load i become fp32 (v_cvt_pk_f32_fp8, exact), are multiplied by the scale of tile i >> 1 (v_mul_f32; the compile
// unit is built without packed fp32 ops) and packed to bf16, round to nearest even (v_cvt_pk_bf16_f32), into bytes 128 i + 32 g4 and + 16
// of the row's image; the two k_pe loads are copied verbatim to bytes 1024 + 64 j + 16 g4. Per lane and step: 64 unpacks, 128 products, 64
// packs, once per workgroup. An empty slot addresses nothing and stages +0 everywhere, its scales included (code 0 is +0, +0 x +0 = +0;
// 0 x garbage in the second product would be NaN).
//
// The image holds FINISHED values, so behind the staging the arithmetic is fa2_decode_paged_mla_sparse_bf16_mfma's statement for statement:
// the score multiplier is softmax_scale log2 e alone and store_split<512> is unscaled. On the pool dequantised to bf16 by the rule above
// that kernel gives the same bits.
//
// The kernel is written ONCE, as a template over the prologue: PACKED = false takes (B, T) and tok = b T + t; PACKED = true takes cu_q and
// finds the sequence of packed row tok by dsav::packed_row (dsa_varlen_row.cuh), a row of no sequence having vis = 0 without a length being
// read: nothing addressed, every step skipped, O = 0, LSE = -inf. With cu_q = [0, T, 2 T, ...] the two give the same bits.
//
// Registers per wave. The budget written before the kernel was the FP8 sibling's about 295 (128 accumulators + 72 Q + 36 rows in flight + 16
// scores + 8 P + fragments, a converted piece, addresses, indices, page, flag words) + 8 more registers of rows in flight + the 16 fp32 of a
// load being staged: about 305 - 320. It was too low: the kernel COMPILES to 412 (256 VGPRs + 156 AGPRs) of the unified 512 under
// __launch_bounds__(256, 1), no spill, no scratch -- and only without packed fp32 ops: with them it needs 424 and spills 6 VGPRs, which is
// why the compile units carry that flag (_build.py). Do not trust the budget, read DESIGN 4.4.26. LDS: the siblings' one image, 64 x 1184
// = 75776 bytes static.
#pragma once
#include "dsa_varlen_row.cuh"
#include "flash_attn_decode_paged_mla_shared.cuh"  // fa2_decode_combine_bf16_all; paged_bf16.cuh

namespace fa2b {

// The siblings' numbers, restated; the compile units assert them against paged_entry.h's.
namespace mlast {
constexpr int kDc = 512, kDr = 64, kDk = kDc + kDr;  // value dims, rotary dims, key dims of a latent row
constexpr int kTile = 128, kTiles = kDc / kTile;     // dims under one scale, scales of a row
constexpr int kScaleByte = kDc;                      // the four fp32 scales of a pool row
constexpr int kPeByte = kScaleByte + 4 * kTiles;     // the 64 bf16 of k_pe
constexpr int kPoolRowBytes = kPeByte + 2 * kDr;     // 656
constexpr int kKeyStep = 64;                         // index slots per workgroup step: four lanes per row, 16 rows per wave
constexpr int kHeadGroup = kWaves * 16;              // query heads of a token per workgroup
constexpr int kRowBytes = 2 * kDk + 32;              // bytes of a latent row in the bf16 LDS image
constexpr int kLdsBytes = kKeyStep * kRowBytes;
constexpr int kFlagByte = 2 * kDk;                   // the first pad byte of a row: the flags of 32 slots in rows 0 and 1
constexpr int kCodeLoads = kDc / 64;                 // 16-byte loads of codes per lane and step: 8
constexpr int kPeLoads = 2 * kDr / 64;               // 16-byte loads of k_pe per lane and step: 2
}  // namespace mlast

// The pool of 656-byte rows [P, page, 656] behind a block table, and the index lists [rows, topk] of logical token positions
struct SparseLatentTile {
  const unsigned char* pool;
  const int *table, *indices;
  int max_pages, page_shift, topk;
  __host__ __device__ int nmax() const { return max_pages << page_shift; }  // the plan checked that it fits
};

// the next step's share of a pool row in flight in a lane
struct TileRow {
  uint4 code[mlast::kCodeLoads];
  f4 scale;
  uint4 pe[mlast::kPeLoads];
};

// 8 codes times the scale of their tile -> 8 bf16: fp32(e4m3) exact, one IEEE fp32 product, one rounding to nearest even
__device__ __forceinline__ b8 e4m3x8_scaled_to_b8(unsigned lo, unsigned hi, float s) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 a0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), a1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f2 a2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), a3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return b8{(bf16_t)(a0[0] * s), (bf16_t)(a0[1] * s), (bf16_t)(a1[0] * s), (bf16_t)(a1[1] * s),
            (bf16_t)(a2[0] * s), (bf16_t)(a2[1] * s), (bf16_t)(a3[0] * s), (bf16_t)(a3[1] * s)};
}

// PACKED = false: rows = T, the tokens of every sequence, tok = b T + t. PACKED = true: rows = total_q, tok = the packed row, B sequences.
template <bool PACKED>
__global__ __launch_bounds__(kThreads, 1) void fa2_decode_paged_mla_sparse_bf16_fp8_tile_mfma(const bf16_t* __restrict__ q, const SparseLatentTile kv,
                                                                                              const int* __restrict__ seqlens,
                                                                                              const int* __restrict__ cu_q, const Out out, int B,
                                                                                              int rows, int Hq, int HG, int S, int C,
                                                                                              float scale_log2) {
  constexpr int DK = mlast::kDk, DV = mlast::kDc;
  constexpr int KS = DK / 32;  // k-steps of S^T: 18
  constexpr int DB = DV / 16;  // 16-dim blocks of O^T: 32
  constexpr int KB = mlast::kKeyStep / 16;  // 16-key blocks of a step: 4
  constexpr int NL = mlast::kCodeLoads, NP = mlast::kPeLoads;
  constexpr int ROW = mlast::kRowBytes, PROW = mlast::kPoolRowBytes;
  static_assert(ROW % 64 == 32 && mlast::kLdsBytes == 75776, "the siblings' image");
  static_assert(mlast::kFlagByte + 32 == ROW && mlast::kKeyStep == 64, "64 flag bytes in the pads of rows 0 and 1");
  static_assert(PROW == 656 && PROW % 16 == 0 && mlast::kScaleByte % 16 == 0 && mlast::kPeByte % 16 == 0, "every load of a row is 16-byte aligned");
  static_assert(NL * 64 == DV && 64 * (NL - 1) + 16 * 3 + 16 == mlast::kScaleByte && 2 * 64 == mlast::kTile, "two loads of a lane per tile, the codes end where the scales begin");
  static_assert(128 * (NL - 1) + 32 * 3 + 32 == 2 * DV && 2 * DV + 64 * (NP - 1) + 16 * 3 + 16 == mlast::kFlagByte, "the staged c ends where k_pe begins, and the image row ends where the flag bytes begin");
  __shared__ __attribute__((aligned(16))) unsigned char smem[mlast::kLdsBytes];

  // the job of workgroup blockIdx.x = (tok HG + hg) S + s: split s of the index list of row tok, for the heads 64 hg ... + 63
  const unsigned job = blockIdx.x / (unsigned)S, s = blockIdx.x - job * (unsigned)S;
  const unsigned tok = job / (unsigned)HG, hg = job - tok * (unsigned)HG;
  unsigned b;
  int vis;  // the dense entry's causal edge
  if constexpr (PACKED) {
    const dsav::PackedRow pr = dsav::packed_row(cu_q, B, rows, tok);
    b = (unsigned)max(pr.b, 0);  // a row of no sequence forms the address of table row 0 and never reads it
    vis = pr.b < 0 ? 0 : min(max(seqlens[b], 0), kv.nmax()) - (pr.T - 1 - pr.t);  // a row of no sequence reads no length
  } else {
    b = tok / (unsigned)rows;
    const unsigned t = tok - b * (unsigned)rows;
    vis = min(max(seqlens[b], 0), kv.nmax()) - (rows - 1 - (int)t);
  }
  const unsigned uvis = (unsigned)max(vis, 0);                            // valid: (unsigned)idx < uvis, a negative idx is a large unsigned
  const unsigned lo = s * (unsigned)C;                                    // (S - 1) C < topk: no overflow
  const unsigned hi = min(lo + (unsigned)C, (unsigned)kv.topk);           // the slots lo ... hi - 1 are this split's
  const unsigned n = hi - lo;                                             // > 0
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int* bt = kv.table + (size_t)b * kv.max_pages;
  const int* ix = kv.indices + (size_t)tok * kv.topk;
  const unsigned pmask = (1u << kv.page_shift) - 1u;
  const int h = (int)hg * mlast::kHeadGroup + 16 * w + i16;              // this lane's query head
  const bool active = (int)hg * mlast::kHeadGroup + 16 * w < Hq;         // wave-uniform: the wave owns a row
  const size_t row = (size_t)tok * Hq + h;                               // flat row of q, o and lse

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
  // an empty slot is not addressed at all: zero codes, zero scales, zero k_pe
  auto load = [&](TileRow& d, int pg, int idx) {
#pragma unroll
    for (int i = 0; i < NL; ++i) d.code[i] = uint4{0u, 0u, 0u, 0u};
    d.scale = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < NP; ++j) d.pe[j] = uint4{0u, 0u, 0u, 0u};
    if (valid(idx)) {
      const unsigned char* src = kv.pool + ((((size_t)pg) << kv.page_shift) + ((unsigned)idx & pmask)) * PROW;
#pragma unroll
      for (int i = 0; i < NL; ++i) d.code[i] = *reinterpret_cast<const uint4*>(src + 64 * i + 16 * g4);
      d.scale = *reinterpret_cast<const f4*>(src + mlast::kScaleByte);
#pragma unroll
      for (int j = 0; j < NP; ++j) d.pe[j] = *reinterpret_cast<const uint4*>(src + mlast::kPeByte + 64 * j + 16 * g4);
    }
  };

  unsigned char* st_p = smem + row0 * ROW + 32 * g4;                                  // where this lane puts its 32 bytes of c of row row0 (+ 128 i bytes)
  unsigned char* pe_p = smem + row0 * ROW + 2 * DV + 16 * g4;                         // ... and its 16 bytes of k_pe (+ 64 j bytes)
  unsigned char* fl_st = smem + (row0 >> 5) * ROW + mlast::kFlagByte + (row0 & 31u);  // the flag byte of slot row0
  const unsigned char* fl_ld = smem + mlast::kFlagByte + 4 * g4;                       // flags of keys 16 kb + 4 g4 ... + 3: + (kb >> 1) ROW + 16 (kb & 1)
  const unsigned char* k_ld = smem + i16 * ROW + 16 * g4;                              // A of S^T: key row 16 kb + i16, dims 32 ks + 8 g4 ...
  const unsigned char* v_ld = smem + (4 * g4 + (i16 >> 2)) * ROW + 8 * (i16 & 3);      // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m = FA2D_NEG_INF, l = 0.0f;
  f4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  TileRow rw;
  int idx = fetch(0), idx2 = fetch(2 * mlast::kKeyStep);  // idx: of the step whose rows are loaded next; idx2: of the step behind it
  int pg = lookup(idx);
  load(rw, pg, idx);
  bool flag = valid(idx);  // of the rows in flight
  idx = fetch(mlast::kKeyStep);
  pg = lookup(idx);
  for (unsigned r0 = 0; r0 < n; r0 += mlast::kKeyStep) {  // n is the workgroup's: every wave takes every barrier
    __syncthreads();  // the reads of the step before are done
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const float sc = rw.scale[i >> 1];  // loads 2 k and 2 k + 1 of a lane lie in tile k
      *reinterpret_cast<b8*>(st_p + 128 * i) = e4m3x8_scaled_to_b8(rw.code[i].x, rw.code[i].y, sc);
      *reinterpret_cast<b8*>(st_p + 128 * i + 16) = e4m3x8_scaled_to_b8(rw.code[i].z, rw.code[i].w, sc);
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) *reinterpret_cast<uint4*>(pe_p + 64 * j) = rw.pe[j];
    if (g4 == 0) *fl_st = flag ? (unsigned char)1 : (unsigned char)0;
    __syncthreads();
    load(rw, pg, idx);  // behind the last step every slot is empty: zeros, no access
    flag = valid(idx);
    pg = lookup(idx2);
    idx = idx2;
    idx2 = fetch(r0 + 3 * mlast::kKeyStep);
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

  // acc[db][e] is dim 16 db + 4 g4 + e of the lane's row. One split: the finished row; more: the raw partial of split s, an empty one
  // included. The head and the row are formed again from a thread index the compiler cannot trace to the one above (an empty asm), as in
  // the FP8 sibling: three registers less that live across the loop
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int he = (int)hg * mlast::kHeadGroup + 16 * (tid >> 6) + (tid & 15), ge = (tid & 63) >> 4;
  const size_t rowe = (size_t)tok * Hq + he;
  if (he < Hq) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) store_split<DV>(out, rowe, 16 * db + 4 * ge + e, s, S, m, l, acc[db][e]);
  }
}

// launch_decode_paged_mla_sparse with the pool of 656-byte rows: the same grid, the same combine. PACKED = false: (B, rows = T); true:
// (B, rows = total_q) and cu_q.
template <bool PACKED>
int launch_decode_paged_mla_sparse_fp8_tile(const void* q, const SparseLatentTile& kv, const int* seqlens, const int* cu_q, void* o, float* lse,
                                            void* workspace, int B, int rows, int Hq, int S, int C, float scale_log2, hipStream_t stream) {
  const int HG = (Hq + mlast::kHeadGroup - 1) / mlast::kHeadGroup;
  const long long toks = PACKED ? (long long)rows : (long long)B * rows, orows = toks * Hq;
  const Out out = make_out(o, lse, workspace, orows, S, mlast::kDc);
  CLN_LAUNCH((fa2_decode_paged_mla_sparse_bf16_fp8_tile_mfma<PACKED>), dim3((unsigned)(toks * HG * S)), dim3(kThreads), 0, stream,
             (const bf16_t*)q, kv, seqlens, cu_q, out, B, rows, Hq, HG, S, C, scale_log2);
  const int rc = cln_check_launch();
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_combine_bf16_all<mlast::kDc>), dim3((unsigned)orows), dim3(mlast::kDc), 0, stream, (const float*)out.ws_o,
             (const float*)out.ws_ml, out.o, out.lse, S);
  return cln_check_launch();
}

}  // namespace fa2b
