// Prefill attention over a PAGED KV cache for a PACKED batch with a per-sequence number of new tokens (cln_fa2_prefill_paged_varlen,
// include/cln_amd_ext.h): flash_attn_prefill_paged.cuh with T replaced per sequence by T_b = cu_q[b + 1] - cu_q[b],
//   O[cu_q[b] + t, h, :] = sum_{j < n(b,t)} softmax_j(q[cu_q[b] + t, h] . K_j / sqrt(D)) V_j,   n(b,t) = len_b - (T_b - 1 - t).
// q, o fp16 [total_q,Hq,D]; cu_q int32 [B + 1] ON THE DEVICE, like the table and the lengths (the host reads none of them); packed rows below
// cu_q[0] or at and past cu_q[B] belong to no sequence and are neither read nor written. The kernel is a SIBLING of
// fa2pp::fa2_prefill_paged_kernel -- its body behind another prologue, softmax_step and the constants shared: the tiles of a sequence start at the
// sequence's own row 0 with rows r = t G + g, so the summation order of a row is fixed by its position in its sequence alone and its bits are
// those of the fixed-T entry on that sequence.
//
// One launch, no plan kernel, no workspace: per KV head the grid has slots = total_q G / 128 + B workgroups (rounded down), and sequence b owns
// the slots from s_b = cu_q[b] G / 128 + b (rounded down). floor((x + y) / 128) >= floor(x / 128) + floor(y / 128) gives
// s_{b+1} >= s_b + ceil(T_b G / 128): the ranges are disjoint, s is strictly increasing (also across empty sequences), every tile has a slot
// below `slots`, and at most B slots per KV head are empty. A workgroup finds the largest b with s_b <= its slot by BINARY SEARCH,
// ceil(log2(B + 1)) dependent scalar loads of cu_q, and returns when its tile lies behind the sequence's last.
//
// A malformed cu_q (decreasing, or values outside [0, total_q]) is outside the contract but still touches no memory outside the tensors: every
// offset is clamped to [0, total_q] and T_b = max(., 0), so every row this kernel forms is below total_q.
//
// The kernel's name does not end in _kernel: tests/decode_kernels.py and the fp16 surface tests count the *_kernel symbols by the fp16 describe
// texts.
#pragma once
#include "flash_attn_prefill_paged.cuh"

namespace fa2pp {

// first slot of sequence b whose (clamped) first packed row is c; c G < 2^31: the host checked that the grid fits
__device__ __forceinline__ unsigned slot_of(int c, int g_shift, int b) { return (((unsigned)c << g_shift) / (unsigned)kRowTile) + (unsigned)b; }

// The largest b in [0, B) with s_b <= slot, or -1; c0 = its first packed row and T = its token count, both from offsets clamped to [0, total_q].
// Every operand is workgroup-uniform (kernel arguments and blockIdx), so the loads are scalar loads; the result goes through readfirstlane so that
// what depends on it -- the length and the table entries -- stays scalar as well.
__device__ __forceinline__ int seq_of_slot(const int* __restrict__ cu_q, int B, int total_q, int g_shift, unsigned slot, int& c0, int& T) {
  int lo = 0, hi = B;  // s_b <= slot for every b < lo, s_b > slot for every b >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int c = min(max(cu_q[mid], 0), total_q);
    if (slot_of(c, g_shift, mid) <= slot)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int b = __builtin_amdgcn_readfirstlane(lo - 1);
  if (b < 0) return -1;
  c0 = __builtin_amdgcn_readfirstlane(min(max(cu_q[b], 0), total_q));
  T = __builtin_amdgcn_readfirstlane(max(min(max(cu_q[b + 1], 0), total_q) - c0, 0));
  return b;
}

template <int D>
__global__ __launch_bounds__(kThreads, 2) void fa2_prefill_paged_varlen_mfma(const half_t* __restrict__ q, const fa2d::PagedKV kv,
                                                                             const int* __restrict__ seqlens, const int* __restrict__ cu_q,
                                                                             half_t* __restrict__ o, float* __restrict__ lse, int B, int total_q,
                                                                             int g_shift, unsigned slots, float scale_log2) {
  static_assert(D == 64 || D == 128, "head dim");
  constexpr int KS = D / 32;             // k-steps of S^T = the 16-byte pieces a thread stages per step and tensor
  constexpr int DB = D / 16;             // 16-dim blocks of O^T
  constexpr int ROWB = 2 * D + 32;       // bytes of a K or V row in LDS
  constexpr int LPR = D / 8;             // threads per staged row
  constexpr int PASS = kThreads / LPR;   // rows one pass of the workgroup stages
  static_assert(PASS * KS == kKeyStep, "staging covers the step");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kKeyStep * ROWB];
  unsigned char* const sk = smem;
  unsigned char* const sv = smem + kKeyStep * ROWB;

  // workgroup blockIdx.x = h slots + x: slot x of KV head h. The sequence and the tile of a slot: seq_of_slot (workgroup-uniform, scalar loads)
  fa2d::Split sp;
  sp.h = blockIdx.x / slots;
  const unsigned slot = blockIdx.x - sp.h * slots;
  int c0, T;
  const int bs = seq_of_slot(cu_q, B, total_q, g_shift, slot, c0, T);
  if (bs < 0) return;  // a slot in front of the first sequence
  sp.b = (unsigned)bs, sp.bh = sp.b * (unsigned)kv.Hkv + sp.h, sp.s = 0, sp.lo = 0;
  const int G = 1 << g_shift, R = T << g_shift, Hq = kv.Hkv << g_shift;
  const unsigned tile = slot - slot_of(c0, g_shift, bs);
  if (tile >= (unsigned)((R + kRowTile - 1) / kRowTile)) return;               // a slot behind the sequence's last tile (T = 0: every one)
  const int len = min(max(seqlens[sp.b], 0), kv.nmax());
  const int row0 = (int)tile * kRowTile;                                        // < R
  const int rows = min(kRowTile, R - row0);
  const int n_end = len - (T - 1 - ((row0 + rows - 1) >> g_shift));             // the keys the tile's last token sees
  const size_t row_bt = (size_t)c0 * Hq + (size_t)sp.h * G;                     // packed output row of (t, g): row_bt + t Hq + g

  if (n_end <= 0) {  // no row of the tile sees a key
    for (int idx = threadIdx.x; idx < rows * LPR; idx += kThreads) {
      const int r = row0 + idx / LPR;
      const size_t row = row_bt + (size_t)(r >> g_shift) * Hq + (r & (G - 1));
      *reinterpret_cast<h8*>(o + row * D + 8 * (idx % LPR)) = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (lse && idx % LPR == 0) lse[row] = FA2D_NEG_INF;
    }
    return;
  }
  const unsigned n = (unsigned)n_end;

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i16 = lane & 15, g4 = lane >> 4;
  const int wr0 = row0 + w * kWaveRows;  // the wave's first row; wave-uniform from here on
  const int n_wave = wr0 < R ? len - (T - 1 - ((min(wr0 + kWaveRows, R) - 1) >> g_shift)) : 0;  // the keys its last token sees

  // the query fragments, the keys each lane's query sees, and per row tile the keys its first token sees (0 for a tile with rows
  // >= R: those always take the select)
  h8 qf[kMT][KS];
  unsigned nq[kMT], n_tile[kMT];
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    const int rf = wr0 + 16 * qb, r = rf + i16;
    const int t = r >> g_shift, g = r & (G - 1);
    nq[qb] = r < R ? (unsigned)max(len - (T - 1 - t), 0) : 0u;
    n_tile[qb] = rf + 16 <= R ? (unsigned)max(len - (T - 1 - (rf >> g_shift)), 0) : 0u;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      h8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r < R) x = *reinterpret_cast<const h8*>(q + (row_bt + (size_t)t * Hq + g) * D + 32 * ks + 8 * g4);
      qf[qb][ks] = x;
    }
  }

  // staging: this thread's column 8 (tid % LPR) .. + 7 of the rows tid / LPR + PASS i of a step
  const int s_row = threadIdx.x / LPR, s_col = threadIdx.x % LPR;
  const fa2d::PagedKV::At at = kv.at(sp, D, 8 * s_col);
  struct Rows {
    h8 k[KS], v[KS];
  };
  auto lookup = [&](int (&pg)[KS], unsigned k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) pg[i] = kv.lookup(at, k0 + s_row + PASS * i, n);
  };
  auto load = [&](Rows& d, const int (&pg)[KS], unsigned k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const unsigned r = k0 + s_row + PASS * i;
      d.k[i] = h8{0, 0, 0, 0, 0, 0, 0, 0}, d.v[i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (r < n) {
        const size_t e = kv.elem(at, pg[i], r, D);
        d.k[i] = *reinterpret_cast<const h8*>(at.k + e);
        d.v[i] = *reinterpret_cast<const h8*>(at.v + e);
      }
    }
  };
  const int s_off = s_row * ROWB + 16 * s_col;                                          // + PASS i rows
  const unsigned char* k_ld = sk + i16 * ROWB + 16 * g4;                                // + 16 kb rows, + 64 ks bytes
  const unsigned char* v_ld = sv + (4 * g4 + (i16 >> 2)) * ROWB + 8 * (i16 & 3);       // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m[kMT], l[kMT];
  f4 acc[kMT][DB];
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    m[qb] = FA2D_NEG_INF, l[qb] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[qb][db] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  Rows cur;
  int pg[KS];
  lookup(pg, 0);
  load(cur, pg, 0);
  lookup(pg, kKeyStep);
  for (unsigned k0 = 0; k0 < n; k0 += kKeyStep) {
    __syncthreads();  // every wave has read the step before
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      *reinterpret_cast<h8*>(sk + s_off + PASS * i * ROWB) = cur.k[i];
      *reinterpret_cast<h8*>(sv + s_off + PASS * i * ROWB) = cur.v[i];
    }
    __syncthreads();
    Rows nxt;
    load(nxt, pg, k0 + kKeyStep);  // behind the last step every predicate is false: zeros, no access
    lookup(pg, k0 + 2 * kKeyStep);
    if ((int)k0 < n_wave) {  // wave-uniform
      f4 st[kMT][kKB];
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb) {
        h8 kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const h8*>(k_ld + 16 * kb * ROWB + 64 * ks);
#pragma unroll
        for (int qb = 0; qb < kMT; ++qb) {
          st[qb][kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            st[qb][kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[ks], qf[qb][ks], st[qb][kb], 0, 0, 0);
            cln_mfma_keep(st[qb][kb], kf[ks], qf[qb][ks]);
          }
        }
      }
      h8 pf[kMT][2];
#pragma unroll
      for (int qb = 0; qb < kMT; ++qb) {
        float alpha;
        if (k0 + kKeyStep <= n_tile[qb])  // wave-uniform: every key of the step is below the causal edge of every row of the tile
          softmax_step<false>(st[qb], k0 + 4 * g4, nq[qb], scale_log2, m[qb], l[qb], alpha, pf[qb]);
        else
          softmax_step<true>(st[qb], k0 + 4 * g4, nq[qb], scale_log2, m[qb], l[qb], alpha, pf[qb]);
#pragma unroll
        for (int db = 0; db < DB; ++db) acc[qb][db] *= alpha;
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const unsigned char* a = v_ld + 32 * c * ROWB + 32 * db;
          const h8 vf = h8_cat(lds_read_tr16(a), lds_read_tr16(a + 16 * ROWB));
#pragma unroll
          for (int qb = 0; qb < kMT; ++qb) {
            acc[qb][db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[qb][c], acc[qb][db], 0, 0, 0);
            cln_mfma_keep(acc[qb][db], vf, pf[qb][c]);
          }
        }
    }
    cur = nxt;
  }

  // the row sums of the four lanes of a query, in a fixed order (both partners of a swap add the same pair); lane (g4, i16) holds dims
  // 16 db + 4 g4 .. + 3 of query i16
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    float a, c;
    fa2d::swap_pair<16>(l[qb], a, c);
    l[qb] = a + c;
    fa2d::swap_pair<32>(l[qb], a, c);
    l[qb] = a + c;
    const int r = wr0 + 16 * qb + i16;
    if (r < R) {
      const size_t row = row_bt + (size_t)(r >> g_shift) * Hq + (r & (G - 1));
      const float inv = l[qb] > 0.0f ? 1.0f / l[qb] : 0.0f;  // no visible key: O = 0, LSE = -inf
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const f4 x = acc[qb][db] * inv;
        *reinterpret_cast<h4*>(o + row * D + 16 * db + 4 * g4) = h4{(half_t)x[0], (half_t)x[1], (half_t)x[2], (half_t)x[3]};
      }
      if (lse && g4 == 0) lse[row] = l[qb] > 0.0f ? (m[qb] + __builtin_log2f(l[qb])) * 0.6931471805599453f : FA2D_NEG_INF;
    }
  }
}

// slots workgroups per KV head, all in x (the caller checks that the grid fits). No host read of the offsets, the table or the lengths, no
// allocation.
template <int D>
int launch_prefill_paged_varlen(const void* q, const fa2d::PagedKV& kv, const int* seqlens, const int* cu_q, void* o, float* lse, int B,
                                int total_q, int g_shift, long long slots, hipStream_t stream) {
  CLN_LAUNCH((fa2_prefill_paged_varlen_mfma<D>), dim3((unsigned)((long long)kv.Hkv * slots)), dim3(kThreads), 0, stream, (const half_t*)q, kv,
             seqlens, cu_q, (half_t*)o, lse, B, total_q, g_shift, (unsigned)slots, fa2d::scale_log2(D));
  return cln_check_launch();
}

}  // namespace fa2pp
