// Append to a paged LATENT cache (multi-head latent attention) in bf16 for a PACKED batch (cln_kv_append_paged_mla_bf16,
// include/cln_amd_ext.h). A pool row is [c (512) | k_pe (64)], one per token, shared by all query heads; the query rows are
// [q_nope W_UK (512) | q_pe (64)]. The 512 leading dims of either are copied bit for bit, the 64 rotary dims are rotated at the token's
// position. The semantics and the contract are kva::kv_append_paged_varlen_bf16_rows' (kv_append_paged_varlen_bf16.cuh): the cu_q convention,
// token i of sequence b at pos = seqlens[b] - T_b + i, liveness, a token that is not live writes nothing to the pool and zeros to its q_out
// rows, rows of no sequence untouched, q_out may be q. The rotary pieces ARE that unit's kva::move_piece<64, ROPE>, called on the row's rotary
// part: x1 c - x2 s, x1 s + x2 c in fp32 from the bf16 inputs and the fp32 table [max_pos, 64], one rounding. ROPE = 0 copies the rotary dims.
#pragma once
#include "kv_append_paged_varlen_bf16.cuh"

namespace kva {

constexpr int kMlaDc = 512, kMlaDr = 64, kMlaDk = kMlaDc + kMlaDr;

struct ArgsMlaBf16 {
  const bf16_t *c_new, *k_pe_new;  // [total_q,512], [total_q,64]
  bf16_t* pool;                    // [P,page,576]
  const int *table, *seqlens, *cu_q;
  const bf16_t* q;  // [total_q,Hq,576] or null; q_out may be the same pointer
  bf16_t* q_out;
  const float* rope;  // [max_pos,64] or null
  int B, total_q, Hq, P, max_pages, page_shift, max_pos;
};

template <int ROPE>
__global__ __launch_bounds__(kThreads) void kv_append_paged_mla_bf16_rows(const ArgsMlaBf16 a) {
  constexpr unsigned CP = kMlaDc / 8;                               // copied pieces of a row
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
  const int col = j < CP ? (int)(8u * j) : (int)(8u * (j - CP));  // inside the copied part, or inside the rotary part
  if (r == 0) {  // the pool row
    if (!live) return;
    const int pg = a.table[(size_t)b * a.max_pages + (size_t)(pos >> a.page_shift)];
    if ((unsigned)pg >= (unsigned)a.P) return;  // outside the caller's contract: nothing is stored rather than stored out of the pool
    bf16_t* dst = a.pool + ((((size_t)pg) << a.page_shift) + ((size_t)pos & ((1u << a.page_shift) - 1u))) * kMlaDk;
    if (j < CP)
      *(b8*)(dst + col) = *(const b8*)(a.c_new + (size_t)tok * kMlaDc + col);
    else
      move_piece<kMlaDr, ROPE>(a.k_pe_new + (size_t)tok * kMlaDr, dst + kMlaDc, rope, col);
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
int launch_mla_bf16(const ArgsMlaBf16& a, long long y, hipStream_t stream) {
  CLN_LAUNCH((kv_append_paged_mla_bf16_rows<ROPE>), dim3((unsigned)a.total_q, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
