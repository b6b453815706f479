// Multi-head latent attention (MLA) decode over a paged latent cache held in FP8 (OCP e4m3fn) with bf16 queries
// (cln_fa2_decode_paged_mla_bf16_fp8, include/cln_amd_ext.h): the sibling of fa2_decode_paged_mla_bf16_mfma
// (flash_attn_decode_paged_mla_bf16.cuh), whose layout it keeps -- rows over waves, a row group of 64 query rows per workgroup, the 64-key
// step, the ONE LDS image of 64 rows x 1184 bytes in bf16. One pool of codes [P, page, 576] = [c (512) | k_pe (64)], one byte per element, a
// row 576 bytes (every row starts 16-byte aligned), and ONE scale for the whole pool: value = e4m3(code) * kv_scale, kv_scale fp32 [1] on the
// device, finite and > 0, no NaN code in a live row (the caller's contract, as for the other FP8 pools; not checked here).
//
// Staging. Four lanes share a row, as in the sibling; a lane fetches 144 bytes of codes per step, 9 loads of 16 bytes at bytes 64 i + 16 g4 of
// the row, and holds the loads of the next step in 36 registers across the products of this one (the sibling: 72). On the way to LDS it converts
// each 16 codes to 16 bf16 (8 v_cvt_scalef32_pk_bf16_fp8 at scale 2^0, exact: every e4m3 value is a bf16 value) and writes them as two 16-byte
// stores at bytes 128 i + 32 g4 and + 16 of the row's bf16 image: dims 64 i + 16 g4 ... + 15, where the sibling puts them. The conversion runs
// once per workgroup and step, never once per wave: 72 packed conversions per lane and step against 136 MFMAs. A row at or past n of the split is
// not addressed, nor is its table entry; its LDS slot receives zeros (code 0 is +0).
//
// Behind the staging barrier everything is the sibling's, in its order: S^T = K Q^T from plain row reads (72 MFMAs), the mask by select, the
// online softmax, O^T = V^T P^T from transposing reads of dims 0 ... 511 (64 MFMAs). The image holds the UNSCALED codes, so the scale stays out
// of the loop: kv_scale is read once per workgroup, the fp32 score multiplier is (softmax_scale log2 e) kv_scale -- two fp32 products in that
// order -- and kv_scale multiplies the fp32 result in front of its store: the partial O of a split (m and l are in the scores' units already), or
// the finished row O / l. Partials therefore carry the scale and fa2_decode_combine_bf16_rows<512> merges them unchanged. With kv_scale a power
// of two both products are exact, and O and LSE equal the sibling's on the pool dequantised to bf16 bit for bit.
//
// Registers per wave (the budget, written before the kernel; DESIGN 4.4.19 has the compiled numbers): 128 accumulators + 72 Q + 36 of the next
// step's codes + 16 scores + 8 P + K / V fragments in flight, the 8 converted registers of a piece and addresses: about 285, past 256, so
// __launch_bounds__(256, 1) and the unified file of 512. LDS: the sibling's one image, 64 x 1184 = 75776 bytes static.
#pragma once
#include "flash_attn_paged_bf16_fp8_rows.cuh"  // e4m3x8_to_b8; paged_bf16.cuh
#include "flash_attn_decode_paged_mla_shared.cuh"  // store_split_scaled

namespace fa2b {

// The sibling's numbers, restated: its header defines a kernel that is no template, so two compile units cannot both include it. The compile
// unit asserts them against paged_entry.h's, as the sibling's does.
namespace mla8 {
constexpr int kDc = 512, kDr = 64, kDk = kDc + kDr;  // value dims, rotary dims, key dims of a latent row
constexpr int kKeyStep = 64;                         // keys per workgroup step: four lanes per row, 16 rows per wave
constexpr int kRowGroup = kWaves * 16;               // query rows per workgroup
constexpr int kRowBytes = 2 * kDk + 32;              // bytes of a latent row in the bf16 LDS image
constexpr int kLdsBytes = kKeyStep * kRowBytes;
constexpr int kCodeLoads = kDk / 64;                 // 16-byte loads of codes per lane and step: 9
}  // namespace mla8

// The pool of codes [P, page, 576] behind a block table: PagedKV's walk at one byte per element, one "head", no dim offset
struct PagedLatent8 {
  const unsigned char* pool;
  const int* table;
  int max_pages, page_shift;
  __host__ __device__ int nmax() const { return max_pages << page_shift; }  // the plan checked that it fits
};

__global__ __launch_bounds__(kThreads, 1) void fa2_decode_paged_mla_bf16_fp8_mfma(const bf16_t* __restrict__ q, const PagedLatent8 kv,
                                                                                  const int* __restrict__ seqlens,
                                                                                  const float* __restrict__ kv_scale, const Out out, int T, int Hq,
                                                                                  int RG, int S, int C, float scale_log2) {
  constexpr int DK = mla8::kDk, DV = mla8::kDc;
  constexpr int KS = DK / 32;  // k-steps of S^T: 18
  constexpr int DB = DV / 16;  // 16-dim blocks of O^T: 32
  constexpr int KB = mla8::kKeyStep / 16;  // 16-key blocks of a step: 4
  constexpr int NL = mla8::kCodeLoads;
  constexpr int ROW = mla8::kRowBytes;
  static_assert(ROW % 64 == 32 && mla8::kLdsBytes == 75776 && NL * 64 == DK, "the sibling's image; a row of codes is 9 x 4 lanes x 16 bytes");
  __shared__ __attribute__((aligned(16))) unsigned char smem[mla8::kLdsBytes];

  fa2d::Split sp;
  if (!fa2d::split_of(sp, seqlens, RG, kv.nmax(), S, C)) return;  // "heads" = the row groups of a sequence: sp.h is the row group
  const unsigned n = sp.n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int* bt = kv.table + (size_t)sp.b * kv.max_pages;
  const unsigned lo = (unsigned)sp.lo;
  const int R = T * Hq;
  const int r = (int)sp.h * mla8::kRowGroup + 16 * w + i16;  // this lane's query row of the sequence, r = t Hq + h
  const bool active = (int)sp.h * mla8::kRowGroup + 16 * w < R;  // wave-uniform: the wave owns a row
  const size_t row = (size_t)sp.b * R + r;                // flat row of q, o and lse
  const float kvs = *kv_scale;                            // once per workgroup: a uniform load
  const float mult = scale_log2 * kvs;                    // (softmax_scale log2 e) kv_scale

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
  // the physical page of row rr of the split; rows at or past n have no table entry that is ours to read
  auto lookup = [&](unsigned rr) { return rr < n ? bt[(lo + rr) >> kv.page_shift] : 0; };
  // a row at or past n is not addressed at all: zeros
  auto load = [&](uint4(&d)[NL], int pg, unsigned r0) {
    const unsigned rr = r0 + row0;
#pragma unroll
    for (int i = 0; i < NL; ++i) d[i] = uint4{0u, 0u, 0u, 0u};
    if (rr < n) {
      const unsigned char* src = kv.pool + ((((size_t)pg) << kv.page_shift) + ((lo + rr) & ((1u << kv.page_shift) - 1u))) * DK + 16 * g4;
#pragma unroll
      for (int i = 0; i < NL; ++i) d[i] = *reinterpret_cast<const uint4*>(src + 64 * i);
    }
  };

  unsigned char* st_p = smem + row0 * ROW + 32 * g4;                                  // where this lane puts its 32 bytes of row row0 (+ 128 i bytes)
  const unsigned char* k_ld = smem + i16 * ROW + 16 * g4;                              // A of S^T: key row 16 kb + i16, dims 32 ks + 8 g4 ...
  const unsigned char* v_ld = smem + (4 * g4 + (i16 >> 2)) * ROW + 8 * (i16 & 3);      // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m = FA2D_NEG_INF, l = 0.0f;
  f4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  uint4 rows[NL];
  int pg = lookup(row0);  // the physical page of this lane's row of the step, fetched one step ahead of the row
  load(rows, pg, 0);
  pg = lookup(mla8::kKeyStep + row0);
  for (unsigned r0 = 0; r0 < n; r0 += mla8::kKeyStep) {  // n is the workgroup's: every wave takes every barrier
    __syncthreads();  // the reads of the step before are done
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      *reinterpret_cast<b8*>(st_p + 128 * i) = e4m3x8_to_b8(make_uint2(rows[i].x, rows[i].y));
      *reinterpret_cast<b8*>(st_p + 128 * i + 16) = e4m3x8_to_b8(make_uint2(rows[i].z, rows[i].w));
    }
    __syncthreads();
    load(rows, pg, r0 + mla8::kKeyStep);  // behind the last step the predicate is false: zeros, no access
    pg = lookup(r0 + 2 * mla8::kKeyStep + row0);
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
        sc[e] = (key0 + 16 * (e >> 2) + (e & 3) < nql) ? st[e >> 2][e & 3] * mult : FA2D_NEG_INF;
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

  // acc[db][e] is dim 16 db + 4 g4 + e of the lane's row, in units of kv_scale. One split: the finished row; more: the partial of split sp.s
  if (r < R) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) store_split_scaled<DV>(out, row, 16 * db + 4 * g4 + e, sp.s, S, m, l, acc[db][e], kvs);
  }
}

// launch_decode_paged_mla with the pool of codes and its scale: the same grid, the same combine
inline int launch_decode_paged_mla_fp8(const void* q, const PagedLatent8& kv, const int* seqlens, const float* kv_scale, void* o, float* lse,
                                       void* workspace, int B, int T, int Hq, int S, int C, float scale_log2, hipStream_t stream) {
  const int R = T * Hq, RG = (R + mla8::kRowGroup - 1) / mla8::kRowGroup;
  const long long rows = (long long)B * R;
  const Out out = make_out(o, lse, workspace, rows, S, mla8::kDc);
  CLN_LAUNCH(fa2_decode_paged_mla_bf16_fp8_mfma, dim3((unsigned)((long long)B * RG * S)), dim3(kThreads), 0, stream, (const bf16_t*)q, kv, seqlens,
             kv_scale, out, T, Hq, RG, S, C, scale_log2);
  return launch_combine<mla8::kDc>(cln_check_launch(), out, seqlens, rows, R, kv.nmax(), S, C, stream);
}

}  // namespace fa2b
