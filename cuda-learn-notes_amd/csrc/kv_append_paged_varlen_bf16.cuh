// Append to a paged KV cache in bf16 for a PACKED batch (cln_kv_append_paged_varlen_bf16, include/cln_amd_ext.h): the SIBLING of
// kva::kv_append_paged_varlen_rows (kv_append_paged_varlen.cuh, which has the semantics and the contract) with k_new, v_new, q, q_out and the
// pools in bf16. Shared by inclusion: kThreads, the table's load type f4u and grid_y of kv_append_paged.cuh. Repeated with the element type of
// paged_bf16.cuh: the piece mover and the body. The rotation is x1 c - x2 s, x1 s + x2 c in fp32 from the bf16 inputs ((float)bf16 is a 16-bit
// shift: exact) and the fp32 table, rounded once to bf16 (round to nearest even) at the store; V rows and rope = none rows are copied bit for bit.
#pragma once
#include "kv_append_paged.cuh"
#include "paged_bf16.cuh"

namespace kva {

struct ArgsVarlenBf16 {
  const bf16_t *k_new, *v_new;  // [total_q,Hkv,D]
  bf16_t *k_pages, *v_pages;    // [P,Hkv,page,D]
  const int *table, *seqlens, *cu_q;
  const bf16_t* q;  // [total_q,Hq,D] or null; q_out may be the same pointer
  bf16_t* q_out;
  const float* rope;  // [max_pos,D] or null
  int B, total_q, Hq, Hkv, P, max_pages, page_shift, max_pos;
};

// pairs (lo[j], hi[j]) -> (lo c - hi s, lo s + hi c)
__device__ __forceinline__ void rotate8(b8& lo, b8& hi, const float (&c)[8], const float (&s)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x1 = (float)lo[j], x2 = (float)hi[j];
    lo[j] = (bf16_t)(x1 * c[j] - x2 * s[j]);
    hi[j] = (bf16_t)(x1 * s[j] + x2 * c[j]);
  }
}

// kva::move_piece on bf16 rows: the thread's piece(s) of one row, src -> dst (both at the row's start), at column col. rope = the table row of the
// token's position, or null for a plain copy (V rows, ROPE = 0).
template <int D, int ROPE>
__device__ __forceinline__ void move_piece(const bf16_t* src, bf16_t* dst, const float* rope, int col) {
  if constexpr (ROPE == 1) {
    b8 lo = *(const b8*)(src + col), hi = *(const b8*)(src + col + D / 2);
    if (rope) {
      float c[8], s[8];
      const f4u c0 = *(const f4u*)(rope + col), c1 = *(const f4u*)(rope + col + 4);
      const f4u s0 = *(const f4u*)(rope + D / 2 + col), s1 = *(const f4u*)(rope + D / 2 + col + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = c0[j], c[j + 4] = c1[j], s[j] = s0[j], s[j + 4] = s1[j];
      rotate8(lo, hi, c, s);
    }
    *(b8*)(dst + col) = lo;
    *(b8*)(dst + col + D / 2) = hi;
  } else {
    b8 x = *(const b8*)(src + col);
    if (ROPE == 2 && rope) {
      const f4u c = *(const f4u*)(rope + col / 2), s = *(const f4u*)(rope + D / 2 + col / 2);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x1 = (float)x[2 * j], x2 = (float)x[2 * j + 1];
        x[2 * j] = (bf16_t)(x1 * c[j] - x2 * s[j]);
        x[2 * j + 1] = (bf16_t)(x1 * s[j] + x2 * c[j]);
      }
    }
    *(b8*)(dst + col) = x;
  }
}

template <int D, int ROPE>
__global__ __launch_bounds__(kThreads) void kv_append_paged_varlen_bf16_rows(const ArgsVarlenBf16 a) {
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
    bf16_t* dst = (is_v ? a.v_pages : a.k_pages) + row * D;
    move_piece<D, ROPE>(src, dst, is_v ? nullptr : rope, (int)col);
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
int launch_varlen_bf16(const ArgsVarlenBf16& a, long long y, hipStream_t stream) {
  CLN_LAUNCH((kv_append_paged_varlen_bf16_rows<D, ROPE>), dim3((unsigned)a.total_q, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
