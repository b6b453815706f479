// Append to a paged KV cache held in FP8 (OCP e4m3fn) with the rotary embedding fused in (cln_kv_append_paged_fp8, include/cln_amd_ext.h;
// DESIGN 4.4.5): kva::kv_append_paged_kernel (kv_append_paged.cuh) with a quantising store. Tokens, positions, liveness, the grid and the q rows are
// exactly those of the fp16 entry; the pools are one byte per element, [P,Hkv,page,D], and k_scale / v_scale are fp32 [Hkv] on the device. A stored
// byte c of KV head h means e4m3(c) * scale[h].
//
// Per element of a live K or V row, all in IEEE fp32 (the build has no fast-math):
//   inv = 1.0f / scale[h];  z = y * inv;  z clamped to [-448, 448];  byte = e4m3 of z, round to nearest even (v_cvt_pk_fp8_f32)
// with y the fp16 input converted exactly (V, and K without a rotation) or the fp32 rotation result x1 c - x2 s, x1 s + x2 c, NOT rounded to fp16
// in between. The clamp makes the byte independent of what the conversion does on overflow. Scales are finite and > 0 and inputs finite: the
// caller's contract, not checked here.
//
// A thread moves 8 elements of a row (16 bytes in, 8 bytes out) -- with the half-split rotation the two pieces at columns c and c + D/2, so it still
// owns both partners of every pair -- and a q row exactly as kva::move_piece does. No LDS, no atomics, no workspace, one launch.
#pragma once
#include "kv_append_paged.cuh"
#include <stdint.h>

namespace kva {

struct Args8 {
  const half_t *k_new, *v_new;  // [B,T,Hkv,D]
  uint8_t *k_pages, *v_pages;   // [P,Hkv,page,D] e4m3fn
  const int *table, *seqlens;
  const float *k_scale, *v_scale;  // [Hkv]
  const half_t* q;                 // [B,T,Hq,D] or null; q_out may be the same pointer
  half_t* q_out;
  const float* rope;  // [max_pos,D] or null
  int T, Hq, Hkv, P, max_pages, page_shift, max_pos;
};

// 8 floats -> 8 e4m3fn bytes at dst (8-byte aligned): y inv, clamped, rounded to nearest even
__device__ __forceinline__ void store_fp8(uint8_t* dst, const float (&y)[8], float inv) {
  float z[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = fminf(fmaxf(y[j] * inv, -448.0f), 448.0f);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(z[0], z[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(z[2], z[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(z[4], z[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(z[6], z[7], hi, true);
  *(uint2*)dst = make_uint2((unsigned)lo, (unsigned)hi);
}

// The thread's piece(s) of one K or V row, fp16 src -> e4m3 dst (both at the row's start), at column col. rope = the table row of the token's
// position, or null for no rotation (V rows, ROPE = 0).
template <int D, int ROPE>
__device__ __forceinline__ void quantise_piece(const half_t* src, uint8_t* dst, const float* rope, int col, float inv) {
  if constexpr (ROPE == 1) {
    const h8 lo = *(const h8*)(src + col), hi = *(const h8*)(src + col + D / 2);
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
    const h8 x = *(const h8*)(src + col);
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
__global__ __launch_bounds__(kThreads) void kv_append_paged_fp8_kernel(const Args8 a) {
  constexpr unsigned PPR = ROPE == 1 ? D / 16 : D / 8;  // threads per row
  const unsigned tok = blockIdx.x;                      // b T + t
  const unsigned b = tok / (unsigned)a.T, t = tok - b * (unsigned)a.T;
  const unsigned u = blockIdx.y * kThreads + threadIdx.x;
  const unsigned r = u / PPR, col = 8u * (u % PPR);
  const unsigned Hkv = (unsigned)a.Hkv, nq = a.q ? (unsigned)a.Hq : 0u;
  if (r >= 2u * Hkv + nq) return;
  const long long pos = (long long)a.seqlens[b] - a.T + (long long)t;
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
    const half_t* src = (is_v ? a.v_new : a.k_new) + ((size_t)tok * Hkv + h) * D;
    uint8_t* dst = (is_v ? a.v_pages : a.k_pages) + row * D;
    const float inv = 1.0f / (is_v ? a.v_scale : a.k_scale)[h];
    quantise_piece<D, ROPE>(src, dst, is_v ? nullptr : rope, (int)col, inv);
  } else {
    const size_t off = ((size_t)tok * nq + (r - 2u * Hkv)) * D;
    if (live) {
      move_piece<D, ROPE>(a.q + off, a.q_out + off, rope, (int)col);
    } else {  // no output row is left uninitialised
      const h8 z = {};
      *(h8*)(a.q_out + off + col) = z;
      if constexpr (ROPE == 1) *(h8*)(a.q_out + off + col + D / 2) = z;
    }
  }
}

template <int D, int ROPE>
int launch_fp8(const Args8& a, long long tokens, long long y, hipStream_t stream) {
  CLN_LAUNCH((kv_append_paged_fp8_kernel<D, ROPE>), dim3((unsigned)tokens, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
