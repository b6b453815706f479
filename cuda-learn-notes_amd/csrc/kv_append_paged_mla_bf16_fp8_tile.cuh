// Append to a paged LATENT cache (multi-head latent attention) in DeepSeek-V3.2's OWN FP8 row of 656 bytes, for a PACKED batch of bf16 rows
// (cln_kv_append_paged_mla_bf16_fp8_tile, include/cln_amd_ext.h). A pool row, one per token:
//   bytes   0 ... 511   512 e4m3fn codes of the latent c
//   bytes 512 ... 527   4 fp32 scales, one per 128-dim tile of c, for this token
//   bytes 528 ... 655   64 bf16 values of k_pe, rotated, not quantised
// 656 = 41 x 16: every row, its scales and its k_pe are 16-byte aligned. Which row goes where is kva::kv_append_paged_mla_bf16_rows'
// (kv_append_paged_mla_bf16.cuh), word for word: packed rows by cu_q clamped here, seqlens taken after the append, token i of sequence b at
// pos = seqlens[b] - T_b + i, a token that is not live (or whose position has no rope row) writes nothing to the pool and zeros to its q_out
// rows, rows of no sequence untouched, a table entry outside [0, P) stores nothing, q_out may be q. Every pool byte that is not a live
// token's 656 bytes keeps its value.
//
// Per live token and per 128-dim tile of c, all in IEEE fp32, what kv_append_paged_index_bf16_fp8.cuh does per token:
//   scale = cln_fp8_block_scale(max_d |c_d|, pow2)                                 (fp8_block_scale.cuh: max(amax, 1e-4) / 448, pow2 on the bits)
//   inv   = 1.0f / scale
//   code_d = e4m3fn, round to nearest even, of clamp(c_d inv, -448, 448)          (kva::store_fp8, as it stands)
// and the scale is stored as computed. k_pe is rotated in fp32 and rounded once to bf16 by kva::move_piece<64, ROPE>: the bits the bf16 MLA
// append stores; the q rows are that append's too.
//
// The split. Thread u = blockIdx.y 256 + threadIdx.x of token blockIdx.x. u < 64 is ONE WAVE, the first of the token's first workgroup, and
// quantises c: lane j loads 16 bytes (dims 8 j ... 8 j + 7), so a DPP row of 16 lanes is exactly one tile and the tile's amax is the index
// append's four DPP moves inside the row (quad_perm xor 1, xor 2, row_half_mirror, row_mirror); every lane of the row then holds the same
// scale and stores its 8 codes, lane 0 of the row stores the scale. No lane reads an inactive partner: every early return tests tok, b, pos
// or pg, which are the workgroup's, so the 64 lanes leave or stay together. The threads behind them take the 16-byte pieces of k_pe (8, or 4
// with the half-split pairs, which a thread moves two at a time) and then of the Hq query rows, as the bf16 append does. All stores are
// vector stores; no LDS, no atomics, one launch.
#pragma once
#include "fp8_block_scale.cuh"
#include "kv_append_paged_fp8.cuh"  // store_fp8; kv_append_paged.cuh
#include "kv_append_paged_mla_bf16.cuh"

namespace kva {

constexpr int kMlaTile = 128, kMlaTiles = kMlaDc / kMlaTile;
constexpr int kMlaTileScaleByte = kMlaDc, kMlaTilePeByte = kMlaTileScaleByte + 4 * kMlaTiles, kMlaTileRowBytes = kMlaTilePeByte + 2 * kMlaDr;

struct ArgsMlaBf16Fp8Tile {
  const bf16_t *c_new, *k_pe_new;  // [total_q,512], [total_q,64]
  uint8_t* pool;                   // [P,page,656] bytes
  const int *table, *seqlens, *cu_q;
  const bf16_t* q;  // [total_q,Hq,576] or null; q_out may be the same pointer
  bf16_t* q_out;
  const float* rope;  // [max_pos,64] or null
  int B, total_q, Hq, P, max_pages, page_shift, max_pos, pow2;
};

template <int ROPE>
__global__ __launch_bounds__(kThreads) void kv_append_paged_mla_bf16_fp8_tile_rows(const ArgsMlaBf16Fp8Tile a) {
  constexpr unsigned CL = kMlaDc / 8;                                // lanes that quantise c: one wave
  constexpr unsigned PE = ROPE == 1 ? kMlaDr / 16 : kMlaDr / 8;      // threads of k_pe
  constexpr unsigned PPR = kMlaDc / 8 + PE;                          // threads per query row
  static_assert(CL == 64 && kMlaTile / 8 == 16, "c is one wave, a tile one DPP row of 16 lanes");
  static_assert(kMlaTileRowBytes == 656 && kMlaTilePeByte % 16 == 0, "the row, and k_pe 16-byte aligned inside it");
  const unsigned tok = blockIdx.x;  // the packed row, < total_q
  const unsigned u = blockIdx.y * kThreads + threadIdx.x;
  const unsigned nq = a.q ? (unsigned)a.Hq : 0u;
  if (u >= CL + PE + nq * PPR) return;  // never inside the first wave
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
  if (u < CL + PE) {  // the pool row
    if (!live) return;
    const int pg = a.table[(size_t)b * a.max_pages + (size_t)(pos >> a.page_shift)];
    if ((unsigned)pg >= (unsigned)a.P) return;  // outside the caller's contract: nothing is stored rather than stored out of the pool
    uint8_t* dst = a.pool + ((((size_t)pg) << a.page_shift) + ((size_t)pos & ((1u << a.page_shift) - 1u))) * kMlaTileRowBytes;
    if (u >= CL) {
      move_piece<kMlaDr, ROPE>(a.k_pe_new + (size_t)tok * kMlaDr, (bf16_t*)(dst + kMlaTilePeByte), rope, (int)(8u * (u - CL)));
      return;
    }
    // from here on the 64 lanes of the wave are all active; lane u holds dims 8 u ... 8 u + 7 of tile u >> 4
    const b8 x = *(const b8*)(a.c_new + (size_t)tok * kMlaDc + 8u * u);
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
    m = fmaxf(m, cln_dpp<0x140>(m));  // row_mirror: the tile's amax in its 16 lanes
    const float scale = cln_fp8_block_scale(m, a.pow2);
    const float inv = 1.0f / scale;
    store_fp8(dst + 8u * u, y, inv);
    if ((u & 15u) == 0u) *(float*)(dst + kMlaTileScaleByte + 4u * (u >> 4)) = scale;
  } else {  // query head r, piece j: the bf16 append's
    const unsigned v = u - (CL + PE), r = v / PPR, j = v % PPR;
    constexpr unsigned CP = kMlaDc / 8;
    const int col = j < CP ? (int)(8u * j) : (int)(8u * (j - CP));  // inside the copied part, or inside the rotary part
    const size_t off = ((size_t)tok * nq + r) * kMlaDk;
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
int launch_mla_bf16_fp8_tile(const ArgsMlaBf16Fp8Tile& a, long long y, hipStream_t stream) {
  CLN_LAUNCH((kv_append_paged_mla_bf16_fp8_tile_rows<ROPE>), dim3((unsigned)a.total_q, (unsigned)y), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace kva
