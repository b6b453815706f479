// Append bf16 rows of a PACKED batch to a paged KV cache held in FP8 (OCP e4m3fn) with the rotary embedding fused in
// (cln_kv_append_paged_varlen_bf16_fp8, include/cln_amd_ext.h): kva::kv_append_paged_varlen_bf16_rows (kv_append_paged_varlen_bf16.cuh:
// the packed prologue, liveness, the q rows in bf16) with the quantising store of kva::kv_append_paged_fp8_kernel (kv_append_paged_fp8.cuh). The
// pools are one byte per element, [P,Hkv,page,D], and k_scale / v_scale are fp32 [Hkv] on the device. A stored byte c of KV head h means
// e4m3(c) * scale[h].
//
// Per element of a live K or V row, all in IEEE fp32 (the build has no fast-math):
//   inv = 1.0f / scale[h];  z = y * inv;  z clamped to [-448, 448];  byte = e4m3 of z, round to nearest even (v_cvt_pk_fp8_f32)
// with y the bf16 input converted exactly (V, and K without a rotation) or the fp32 rotation result x1 c - x2 s, x1 s + x2 c, NOT rounded to bf16
// in between. Scales are finite and > 0 and inputs finite: the caller's contract, not checked here.
//
// Shared by inclusion: kva::store_fp8, the bf16 kva::move_piece for the q rows, kThreads, f4u, grid_y. Repeated: the piece quantiser for bf16
// sources and the body. A thread moves 8 elements of a row (16 bytes in, 8 bytes out) -- with the half-split rotation the two pieces at columns c
// and c + D/2, so it still owns both partners of every pair. No LDS, no atomics, no workspace, one launch.
#pragma once
#include "kv_append_paged_fp8.cuh"
#include "kv_append_paged_varlen_bf16.cuh"

namespace kva {

struct ArgsVarlenBf16Fp8 {
  const bf16_t *k_new, *v_new;  // [total_q,Hkv,D]
  uint8_t *k_pages, *v_pages;   // [P,Hkv,page,D] e4m3fn
  const int *table, *seqlens, *cu_q;
  const float *k_scale, *v_scale;  // [Hkv]
  const bf16_t* q;                 // [total_q,Hq,D] or null; q_out may be the same pointer
  bf16_t* q_out;
  const float* rope;  // [max_pos,D] or null
  int B, total_q, Hq, Hkv, P, max_pages, page_shift, max_pos;
};

// kva::quantise_piece with a bf16 source: the thread's piece(s) of one K or V row, bf16 src -> e4m3 dst (both at the row's start), at column col.
// rope = the table row of the token's position, or null for no rotation (V rows, ROPE = 0).
template <int D, int ROPE>
__device__ __forceinline__ void quantise_piece(const bf16_t* src, uint8_t* dst, const float* rope, int col, float inv) {
  if constexpr (ROPE == 1) {
    const b8 lo = *(const b8*)(src + col), hi = *(const b8*)(src + col + D / 2);
    float a[8], b[8];
    if (rope) {
      const f4u c0 = *(const f4u*)(rope + col), c1 = *(const f4u*)(rope + col + 4);
      const f4u s0 = *(const f4u*)(rope + D / 2 + col), s1 = *(const f4u*)(rope + D / 2 + col + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = j < 4 ? c0[j & 3] : c1[j & 3], s = j < 4 ? s0[j & 3] : s1[j & 3];
        const float x1 = (float)lo[j], x2 = (float)hi[j];
        a[j] = x1 * c - x2 * s;
        b[j] = x1 * s + x2 * c;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = (float)lo[j], b[j] = (float)hi[j];
    }
    store_fp8(dst + col, a, inv);
    store_fp8(dst + col + D / 2, b, inv);
  } else {
    const b8 x = *(const b8*)(src + col);
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = (float)x[j];
    if (ROPE == 2 && rope) {
      const f4u c = *(const f4u*)(rope + col / 2), s = *(const f4u*)(rope + D / 2 + col / 2);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x1 = (float)x[2 * j], x2 = (float)x[2 * j + 1];
        y[2 * j] = x1 * c[j] - x2 * s[j];
        y[2 * j + 1] = x1 * s[j] + x2 * c[j];
      }
    }
    store_fp8(dst + col, y, inv);
  }
}

template <int D, int ROPE>
__global__ __launch_bounds__(kThreads) void kv_append_paged_varlen_bf16_fp8_rows(const ArgsVarlenBf16Fp8 a) {
  constexpr unsigned PPR = ROPE == 1 ? D / 16 : D / 8;  // threads per row
  const unsigned tok = blockIdx.x;                      // the packed row, < total_q
  const unsigned u = blockIdx.y * kThreads + threadIdx.x;
  const unsigned r = u / PPR, col = 8u * (u % PPR);
  const unsigned Hkv = (unsigned)a.Hkv, nq = a.q ? (unsigned)a.Hq : 0u;
  if (r >= 2u * Hkv + nq) return;
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
  const float* rope = ROPE != 0 && live ? a.rope + (size_t)pos * D : nullptr;
  if (r < 2u * Hkv) {  // a K row (r < Hkv) or a V row of the pool
    if (!live) return;
    const int pg = a.table[(size_t)b * a.max_pages + (size_t)(pos >> a.page_shift)];
    if ((unsigned)pg >= (unsigned)a.P) return;  // outside the caller's contract: nothing is stored rather than stored out of the pool
    const bool is_v = r >= Hkv;
    const unsigned h = is_v ? r - Hkv : r;
    const size_t row = (((size_t)pg * Hkv + h) << a.page_shift) + ((size_t)pos & ((1u << a.page_shift) - 1u));
    const bf16_t* src = (is_v ? a.v_new : a.k_new) + ((size_t)tok * Hkv + h) * D;
    uint8_t* dst = (is_v ? a.v_pages : a.k_pages) + row * D;
    const float inv = 1.0f / (is_v ? a.v_scale : a.k_scale)[h];
    quantise_piece<D, ROPE>(src, dst, is_v ? nullptr : rope, (int)col, inv);
  } else {
    const size_t off = ((size_t)tok * nq + (r - 2u * Hkv)) * D;
    if (live) {
      move_piece<D, ROPE>(a.q + off, a.q_out + off, rope, (int)col);
    } else {  // no output row of a sequence is left uninitialised
      const b8 z = {};
      *(b8*)(a.q_out + off + col) = z;
      if constexpr (ROPE == 1) *(b8*)(a.q_out + off + col + D / 2) = z;
    }
  }
}

template <int D, int ROPE>
int launch_varlen_bf16_fp8(const ArgsVarlenBf16Fp8& a, long long y, hipStream_t stream) {
  CLN_LAUNCH((kv_append_paged_varlen_bf16_fp8_rows<D, ROPE>), dim3((unsigned)a.total_q, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
