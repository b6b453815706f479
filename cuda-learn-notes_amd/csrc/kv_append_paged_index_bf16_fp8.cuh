// Append to the paged INDEX-KEY cache of DeepSeek-V3.2's indexer held in FP8 (OCP e4m3fn) with ONE fp32 SCALE PER TOKEN, for a PACKED batch of
// bf16 keys (cln_kv_append_paged_index_bf16_fp8, include/cln_amd_ext.h). Which row goes where is
// kva::kv_append_paged_index_bf16_rows' (kv_append_paged_index_bf16.cuh), word for word: packed rows by cu_q clamped here, seqlens taken after
// the append, token i of sequence b at pos = seqlens[b] - T_b + i, a token that is not live writes nothing, rows of no sequence untouched, a
// table entry outside [0, P) stores nothing. No rotation, for the reason given there.
//
// The pool is bytes, [P, page, 132] to the caller; inside a page of 132 page bytes the codes come first and the scales behind them:
//   bytes [0, 128 page)          codes [page, 128] e4m3fn, slot r at byte 128 r
//   bytes [128 page, 132 page)   scales [page] fp32,      slot r at byte 128 page + 4 r
// 132 page is a multiple of 16 for every supported page (16 ... 256), so a code row is 16-byte aligned and a scale 4-byte aligned. A stored
// token means k_d = e4m3(code_d) scale. Every byte that is not a live token's 128 codes or 4 scale bytes keeps its value.
//
// Per live token, all in IEEE fp32 (the build has no fast-math; bf16 is exact in fp32):
//   a     = max(max_d |k_d|, 1e-4f)
//   scale = a / 448.0f
//   if pow2: scale = the smallest power of two >= scale -- on the bits: mantissa zero -> unchanged, else exponent + 1, mantissa 0 (no log2)
//   inv   = 1.0f / scale
//   code_d = e4m3fn, round to nearest even, of clamp(k_d inv, -448, 448)          (kva::store_fp8, as it stands)
// and the scale is stored as computed. Inputs are finite: the caller's contract. scale >= 1e-4 / 448 > 0 always.
//
// 16 threads a row: a thread loads 16 bytes (8 dims), takes their largest magnitude, and the row's amax goes over its 16 lanes by four DPP
// moves inside the 16-lane row (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: after them every lane holds the row's maximum; max is
// exact, so the order is immaterial). No lane reads an inactive partner: u = 16 tok + j with j = lane & 15, so the 16 lanes of a DPP row are
// the 16 pieces of ONE packed row, and every early return below -- tok >= total_q, no sequence, not live, a table entry outside [0, P) --
// tests tok, b, pos or pg only, never j: the 16 lanes of a row leave or stay together, and the moves never cross a row. Every lane then
// computes the same scale and stores its 8 codes; lane 0 of the row stores the scale. No LDS, no atomics, one launch.
#pragma once
#include "kv_append_paged_fp8.cuh"  // store_fp8; kv_append_paged.cuh
#include "paged_bf16.cuh"

namespace kva {

constexpr int kIdx8Dim = 128, kIdx8RowBytes = 132;

struct ArgsIndexBf16Fp8 {
  const bf16_t* k_new;  // [total_q,128]
  uint8_t* pool;        // [P, 132 page] bytes: codes [page,128], then scales [page] fp32
  const int *table, *seqlens, *cu_q;
  int B, total_q, P, max_pages, page_shift, pow2;
};

__global__ __launch_bounds__(kThreads) void kv_append_paged_index_bf16_fp8_rows(const ArgsIndexBf16Fp8 a) {
  constexpr unsigned PPR = kIdx8Dim / 8;  // pieces = threads per row: one DPP row of 16 lanes
  static_assert(PPR == 16, "the amax runs over a DPP row");
  const unsigned u = blockIdx.x * kThreads + threadIdx.x;
  const unsigned tok = u / PPR, j = u % PPR;  // the packed row and the piece
  if (tok >= (unsigned)a.total_q) return;
  // the largest b in [0, B) whose clamped offset is <= tok
  int lo = 0, hi = a.B;  // offset <= tok for every b < lo, > tok for every b >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)min(max(a.cu_q[mid], 0), a.total_q) <= tok)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int b = lo - 1;
  if (b < 0) return;  // a row in front of the first sequence
  const int c0 = min(max(a.cu_q[b], 0), a.total_q);
  const int T = max(min(max(a.cu_q[b + 1], 0), a.total_q) - c0, 0);
  const unsigned t = tok - (unsigned)c0;
  if (t >= (unsigned)T) return;  // a row behind the last sequence
  const long long pos = (long long)a.seqlens[b] - T + (long long)t;
  if (pos < 0 || pos >= ((long long)a.max_pages << a.page_shift)) return;  // not live
  const int pg = a.table[(size_t)b * a.max_pages + (size_t)(pos >> a.page_shift)];
  if ((unsigned)pg >= (unsigned)a.P) return;  // outside the caller's contract: nothing is stored rather than stored out of the pool
  // from here on the 16 lanes of the row are all active
  const b8 x = *(const b8*)(a.k_new + (size_t)tok * kIdx8Dim + 8u * j);
  float y[8];
  float m = 0.0f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    y[e] = (float)x[e];
    m = fmaxf(m, fabsf(y[e]));
  }
  m = fmaxf(m, cln_dpp<0xB1>(m));   // quad_perm [1,0,3,2]
  m = fmaxf(m, cln_dpp<0x4E>(m));   // quad_perm [2,3,0,1]
  m = fmaxf(m, cln_dpp<0x141>(m));  // row_half_mirror
  m = fmaxf(m, cln_dpp<0x140>(m));  // row_mirror: the row's amax in its 16 lanes
  float scale = fmaxf(m, 1e-4f) / 448.0f;
  if (a.pow2) {
    const unsigned bits = __float_as_uint(scale);  // positive and normal
    if (bits & 0x007fffffu) scale = __uint_as_float((bits & 0x7f800000u) + 0x00800000u);
  }
  const float inv = 1.0f / scale;
  const size_t r = (size_t)pos & ((1u << a.page_shift) - 1u);
  uint8_t* pagep = a.pool + (size_t)pg * ((size_t)kIdx8RowBytes << a.page_shift);
  store_fp8(pagep + r * kIdx8Dim + 8u * j, y, inv);
  if (j == 0) *(float*)(pagep + ((size_t)kIdx8Dim << a.page_shift) + 4u * r) = scale;
}

inline int launch_index_bf16_fp8(const ArgsIndexBf16Fp8& a, long long wgs, hipStream_t stream) {
  CLN_LAUNCH(kv_append_paged_index_bf16_fp8_rows, dim3((unsigned)wgs), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
