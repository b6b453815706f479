// Append to a paged KV cache with the rotary embedding fused in (cln_kv_append_paged, include/cln_amd_ext.h): the first two thirds
// of a decode step -- rotate q and k, write the new K / V rows into the pool -- as one launch, in the conventions of the paged attention entries
// (flash_attn_decode_common.cuh): pools fp16 [P,Hkv,page,D], block table int32 [B,max_pages], seqlens int32 [B] that count the T new tokens.
//
// Token t of sequence b stands at pos = seqlens[b] - T + t (formed in 64 bits: any int32 length is safe). It is live iff 0 <= pos < max_pages page
// and, with a rotation, pos < max_pos. A live token's K and V rows of every KV head go to row pos % page of page block_table[b, pos / page]; a
// token that is not live writes nothing to the pools and zeros to its q_out rows.
//
// Work: a token has 2 Hkv pool rows and, with q, Hq query rows of D halves. A thread moves one 16-byte piece of one row -- with the half-split
// rotation (ROPE = 1) the two pieces at columns c and c + D/2, whose elements are each other's partners -- so it owns both elements of every pair it
// touches and reads them before it writes: q_out may be q. Workgroup (x, y) serves pieces [256 y, 256 y + 256) of token x: the length and the table
// entry of a workgroup are uniform and come through scalar loads. The rotation is x1 c - x2 s, x1 s + x2 c in fp32 from a caller's table
// (row p: cos(p f_i) for i < D/2, then sin(p f_i)), rounded once at the store. The pool stores are plain: the attention call that follows reads
// these rows, so they should stay in L2. No LDS, no atomics, no workspace.
#pragma once
#include "common.h"

namespace kva {

constexpr int kThreads = 256;

// the table is only 4-byte aligned (a row of a caller's larger table, a sliced view): dwordx4 loads that promise no more than that
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

struct Args {
  const half_t *k_new, *v_new;  // [B,T,Hkv,D]
  half_t *k_pages, *v_pages;    // [P,Hkv,page,D]
  const int *table, *seqlens;
  const half_t* q;  // [B,T,Hq,D] or null; q_out may be the same pointer
  half_t* q_out;
  const float* rope;  // [max_pos,D] or null
  int T, Hq, Hkv, P, max_pages, page_shift, max_pos;
};

// pairs (lo[j], hi[j]) -> (lo c - hi s, lo s + hi c)
__device__ __forceinline__ void rotate8(h8& lo, h8& hi, const float (&c)[8], const float (&s)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x1 = (float)lo[j], x2 = (float)hi[j];
    lo[j] = (half_t)(x1 * c[j] - x2 * s[j]);
    hi[j] = (half_t)(x1 * s[j] + x2 * c[j]);
  }
}

// The thread's piece(s) of one row, src -> dst (both at the row's start), at column col. rope = the table row of the token's position, or null for
// a plain copy (V rows, ROPE = 0).
template <int D, int ROPE>
__device__ __forceinline__ void move_piece(const half_t* src, half_t* dst, const float* rope, int col) {
  if constexpr (ROPE == 1) {
    h8 lo = *(const h8*)(src + col), hi = *(const h8*)(src + col + D / 2);
    if (rope) {
      float c[8], s[8];
      const f4u c0 = *(const f4u*)(rope + col), c1 = *(const f4u*)(rope + col + 4);
      const f4u s0 = *(const f4u*)(rope + D / 2 + col), s1 = *(const f4u*)(rope + D / 2 + col + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = c0[j], c[j + 4] = c1[j], s[j] = s0[j], s[j + 4] = s1[j];
      rotate8(lo, hi, c, s);
    }
    *(h8*)(dst + col) = lo;
    *(h8*)(dst + col + D / 2) = hi;
  } else {
    h8 x = *(const h8*)(src + col);
    if (ROPE == 2 && rope) {
      const f4u c = *(const f4u*)(rope + col / 2), s = *(const f4u*)(rope + D / 2 + col / 2);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x1 = (float)x[2 * j], x2 = (float)x[2 * j + 1];
        x[2 * j] = (half_t)(x1 * c[j] - x2 * s[j]);
        x[2 * j + 1] = (half_t)(x1 * s[j] + x2 * c[j]);
      }
    }
    *(h8*)(dst + col) = x;
  }
}

template <int D, int ROPE>
__global__ __launch_bounds__(kThreads) void kv_append_paged_kernel(const Args a) {
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
    half_t* dst = (is_v ? a.v_pages : a.k_pages) + row * D;
    move_piece<D, ROPE>(src, dst, is_v ? nullptr : rope, (int)col);
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

// y workgroups per token; 0 when the grid does not fit (x: B T workgroups of 256 threads, y: at most 65535)
inline long long grid_y(long long B, long long T, long long Hq, long long Hkv, bool has_q, int D, int rope_mode) {
  const long long units = (2 * Hkv + (has_q ? Hq : 0)) * (rope_mode == 1 ? D / 16 : D / 8);
  const long long y = (units + kThreads - 1) / kThreads;
  return B * T <= 0xffffffffLL / kThreads && y <= 65535 ? y : 0;
}

template <int D, int ROPE>
int launch(const Args& a, long long tokens, long long y, hipStream_t stream) {
  CLN_LAUNCH((kv_append_paged_kernel<D, ROPE>), dim3((unsigned)tokens, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
