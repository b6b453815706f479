// Append to a paged LATENT cache (multi-head latent attention) held in FP8 (OCP e4m3fn) for a PACKED batch of bf16 rows
// (cln_kv_append_paged_mla_bf16_fp8, include/cln_amd_ext.h): kva::kv_append_paged_mla_bf16_rows (kv_append_paged_mla_bf16.cuh:
// the packed prologue, liveness, clamping, the q rows in bf16, rows of no sequence untouched) with the quantising store of
// kva::kv_append_paged_varlen_bf16_fp8_rows (kv_append_paged_varlen_bf16_fp8.cuh). The pool is one byte per element, [P,page,576], a row
// [c (512) | k_pe (64)] in codes, and kv_scale is fp32 [1] on the device, ONE scale for the whole row: a stored byte c means e4m3(c) * kv_scale.
//
// Per element of a live pool row, all in IEEE fp32 (the build has no fast-math):
//   inv = 1.0f / kv_scale;  z = y * inv;  z clamped to [-448, 448];  byte = e4m3 of z, round to nearest even (v_cvt_pk_fp8_f32)
// with y the bf16 input converted exactly (c, and k_pe without a rotation) or the fp32 rotation result x1 c - x2 s, x1 s + x2 c, NOT rounded to
// bf16 in between. The pieces ARE kva::quantise_piece (bf16 source): <512, 0> on c, <64, ROPE> on k_pe. The q rows are the bf16 MLA append's:
// dims 0 ... 511 copied, 512 ... 575 moved by kva::move_piece<64, ROPE>, bf16. A thread moves 8 elements of a row (16 bytes in, 8 bytes out into
// the pool) -- with the half-split rotation the two pieces at columns c and c + 32. The launch shape is the bf16 MLA append's.
#pragma once
#include "kv_append_paged_mla_bf16.cuh"
#include "kv_append_paged_varlen_bf16_fp8.cuh"

namespace kva {

struct ArgsMlaBf16Fp8 {
  const bf16_t *c_new, *k_pe_new;  // [total_q,512], [total_q,64]
  uint8_t* pool;                   // [P,page,576] e4m3fn
  const int *table, *seqlens, *cu_q;
  const float* kv_scale;  // [1]
  const bf16_t* q;        // [total_q,Hq,576] or null; q_out may be the same pointer
  bf16_t* q_out;
  const float* rope;  // [max_pos,64] or null
  int B, total_q, Hq, P, max_pages, page_shift, max_pos;
};

template <int ROPE>
__global__ __launch_bounds__(kThreads) void kv_append_paged_mla_bf16_fp8_rows(const ArgsMlaBf16Fp8 a) {
  constexpr unsigned CP = kMlaDc / 8;                               // quantised (q: copied) pieces of a row
  constexpr unsigned PPR = CP + (ROPE == 1 ? kMlaDr / 16 : kMlaDr / 8);  // threads per row
  const unsigned tok = blockIdx.x;                                  // the packed row, < total_q
  const unsigned u = blockIdx.y * kThreads + threadIdx.x;
  const unsigned r = u / PPR, j = u % PPR;                          // row 0: the pool row; 1 + h: query head h
  const unsigned nq = a.q ? (unsigned)a.Hq : 0u;
  if (r >= 1u + nq) return;
  // the largest b in [0, B) whose clamped offset is <= tok
  int lo = 0, hi = a.B;  // offset <= tok for every b < lo, > tok for every b >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)min(max(a.cu_q[mid], 0), a.total_q) <= tok)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int b = __builtin_amdgcn_readfirstlane(lo - 1);
  if (b < 0) return;  // a row in front of the first sequence
  const int c0 = __builtin_amdgcn_readfirstlane(min(max(a.cu_q[b], 0), a.total_q));
  const int T = __builtin_amdgcn_readfirstlane(max(min(max(a.cu_q[b + 1], 0), a.total_q) - c0, 0));
  const unsigned t = tok - (unsigned)c0;
  if (t >= (unsigned)T) return;  // a row behind the last sequence
  const long long pos = (long long)a.seqlens[b] - T + (long long)t;
  bool live = pos >= 0 && pos < ((long long)a.max_pages << a.page_shift);
  if (ROPE != 0) live = live && pos < (long long)a.max_pos;
  const float* rope = ROPE != 0 && live ? a.rope + (size_t)pos * kMlaDr : nullptr;
  const int col = j < CP ? (int)(8u * j) : (int)(8u * (j - CP));  // inside the leading part, or inside the rotary part
  if (r == 0) {  // the pool row
    if (!live) return;
    const int pg = a.table[(size_t)b * a.max_pages + (size_t)(pos >> a.page_shift)];
    if ((unsigned)pg >= (unsigned)a.P) return;  // outside the caller's contract: nothing is stored rather than stored out of the pool
    uint8_t* dst = a.pool + ((((size_t)pg) << a.page_shift) + ((size_t)pos & ((1u << a.page_shift) - 1u))) * kMlaDk;
    const float inv = 1.0f / a.kv_scale[0];
    if (j < CP)
      quantise_piece<kMlaDc, 0>(a.c_new + (size_t)tok * kMlaDc, dst, nullptr, col, inv);
    else
      quantise_piece<kMlaDr, ROPE>(a.k_pe_new + (size_t)tok * kMlaDr, dst + kMlaDc, rope, col, inv);
  } else {
    const size_t off = ((size_t)tok * nq + (r - 1u)) * kMlaDk;
    if (j < CP) {
      b8 x = {};
      if (live) x = *(const b8*)(a.q + off + col);
      *(b8*)(a.q_out + off + col) = x;  // no output row of a sequence is left uninitialised
    } else if (live) {
      move_piece<kMlaDr, ROPE>(a.q + off + kMlaDc, a.q_out + off + kMlaDc, rope, col);
    } else {
      const b8 z = {};
      *(b8*)(a.q_out + off + kMlaDc + col) = z;
      if constexpr (ROPE == 1) *(b8*)(a.q_out + off + kMlaDc + col + kMlaDr / 2) = z;
    }
  }
}

template <int ROPE>
int launch_mla_bf16_fp8(const ArgsMlaBf16Fp8& a, long long y, hipStream_t stream) {
  CLN_LAUNCH((kv_append_paged_mla_bf16_fp8_rows<ROPE>), dim3((unsigned)a.total_q, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
