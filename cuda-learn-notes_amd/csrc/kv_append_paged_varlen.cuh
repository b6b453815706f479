// Append to a paged KV cache for a PACKED batch with a per-sequence number of new tokens (cln_kv_append_paged_varlen, include/cln_amd_ext.h;
// DESIGN 4.4.7): kva::kv_append_paged_kernel (kv_append_paged.cuh) with T replaced per sequence by T_b = cu_q[b + 1] - cu_q[b]. k_new, v_new fp16
// [total_q,Hkv,D], q / q_out fp16 [total_q,Hq,D]; cu_q int32 [B + 1] ON THE DEVICE, like the table and the lengths. Token t of sequence b is packed
// row cu_q[b] + t and stands at pos = seqlens[b] - T_b + t (64 bits); liveness, the page arithmetic, the pieces and the zero fill of the q_out rows
// of tokens that are not live are the sibling's (move_piece, rotate8 and the table's load type are shared, not repeated).
//
// Workgroup (x, y) serves pieces [256 y, 256 y + 256) of PACKED ROW x. Its sequence is the largest b with cu_q[b] <= x, found by binary search:
// ceil(log2(B + 1)) dependent scalar loads, every operand workgroup-uniform. A row below cu_q[0] or at and past cu_q[B] belongs to no sequence:
// the workgroup returns without a load or a store of a tensor row. A malformed cu_q (decreasing, values outside [0, total_q]) is outside the
// contract; the offsets are clamped to [0, total_q] and T_b = max(., 0), and the only rows touched are row x < total_q of the packed tensors.
//
// The kernel's name does not end in _kernel: the fp16 surface test counts the *_kernel symbols of its own compile unit.
#pragma once
#include "kv_append_paged.cuh"

namespace kva {

struct ArgsVarlen {
  const half_t *k_new, *v_new;  // [total_q,Hkv,D]
  half_t *k_pages, *v_pages;    // [P,Hkv,page,D]
  const int *table, *seqlens, *cu_q;
  const half_t* q;  // [total_q,Hq,D] or null; q_out may be the same pointer
  half_t* q_out;
  const float* rope;  // [max_pos,D] or null
  int B, total_q, Hq, Hkv, P, max_pages, page_shift, max_pos;
};

template <int D, int ROPE>
__global__ __launch_bounds__(kThreads) void kv_append_paged_varlen_rows(const ArgsVarlen a) {
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
    const half_t* src = (is_v ? a.v_new : a.k_new) + ((size_t)tok * Hkv + h) * D;
    half_t* dst = (is_v ? a.v_pages : a.k_pages) + row * D;
    move_piece<D, ROPE>(src, dst, is_v ? nullptr : rope, (int)col);
  } else {
    const size_t off = ((size_t)tok * nq + (r - 2u * Hkv)) * D;
    if (live) {
      move_piece<D, ROPE>(a.q + off, a.q_out + off, rope, (int)col);
    } else {  // no output row of a sequence is left uninitialised
      const h8 z = {};
      *(h8*)(a.q_out + off + col) = z;
      if constexpr (ROPE == 1) *(h8*)(a.q_out + off + col + D / 2) = z;
    }
  }
}

template <int D, int ROPE>
int launch_varlen(const ArgsVarlen& a, long long y, hipStream_t stream) {
  CLN_LAUNCH((kv_append_paged_varlen_rows<D, ROPE>), dim3((unsigned)a.total_q, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
