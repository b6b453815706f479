// Packed variable-length prefill attention over a PAGED KV cache in bf16 at HEAD DIM 256, with a sliding window, optional attention sinks, any
// query-group size G = Hq / Hkv in 1 ... 16, a softmax scale of the caller's and optional logit soft-capping
// (cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16, include/cln_amd_ext.h): the SIBLING of
// fa2b::fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_mfma (flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_bf16.cuh), which
// takes D = 64 and 128. The semantics, the masks, the order cap -> mask, the sink and the epilogue are that kernel's.
//
// The budget that decides the layout (registers per lane, 32-bit; DESIGN 4.4.16 has the table with the compiler's numbers):
//   per 16-row tile   64 accumulators (16 f4), 32 of Q fragments (8 b8), 16 of scores (4 f4), 8 of P (2 b8)
//   per thread        a 64-key step staged through registers: 8 pieces of 16 bytes per tensor = 32 for K and 32 for V, live from the load in
//                     one step to the LDS store in the next; 32 of K fragments (8 b8) per 16-key block while the scores are formed
// The workgroup tile stays 128 rows -- four waves of two 16-row tiles, kMT = 2 -- so seq_of_slot_anyg, slot_of_anyg and slots = total_q G / 128 + B
// serve unchanged and a staged K / V step feeds 128 rows as at D = 128: 2 (64 + 32 + 16 + 8) + 64 + 32 = 336 registers before addresses and the
// softmax temporaries. That is past the 256 architectural VGPRs, so the kernel asks for one wave per SIMD (__launch_bounds__(256, 1)), which on
// gfx950 gives a wave the unified file of 512: the MFMA accumulators take AGPRs as their C / D operand directly, and nothing is spilled. The
// alternative, a 64-row tile at two waves per SIMD, halves the rows a staged step feeds (every K fragment read from LDS then feeds one MFMA
// instead of two) and needs slot helpers of its own; it was not taken. MEASURED: this layout runs at 2.1 - 5.7 times the
// D = 128 kernel's time where 2.0 was the reference point -- one wave per SIMD costs more than the shared tile saves. A layout at two waves per
// SIMD (eight waves of one 16-row tile on this same tile and LDS image, or the 64-row tile) is the next step.
// LDS: K and V of a 64-key step in rows of 2 D + 32 = 544 bytes (the padding that keeps the transposing reads off each other's banks):
// 2 x 64 x 544 = 69632 bytes, static. One workgroup per CU.
// Per step and wave: 4 key blocks x 2 row tiles x 8 k-steps = 64 MFMAs for S^T and 2 x 16 dim blocks x 2 row tiles = 64 for O^T, all
// v_mfma_f32_16x16x32_bf16.
// Shared by inclusion: everything the sibling shares. Repeated: the body.
#pragma once
#include "flash_attn_prefill_paged_varlen_window_sink_softcap_anyg_bf16.cuh"

namespace fa2b {

constexpr int kHeadDim256 = 256;
constexpr int kPrefill256LdsBytes = 2 * kKeyStep * (2 * kHeadDim256 + 32);

template <bool CAP>
__global__ __launch_bounds__(kThreads, 1) void fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_mfma(
    const bf16_t* __restrict__ q, const PagedKV kv, const int* __restrict__ seqlens, const int* __restrict__ cu_q, const float* __restrict__ sinks,
    bf16_t* __restrict__ o, float* __restrict__ lse, int B, int total_q, int G, unsigned slots, int W, float scale_log2, float pre, float cap2) {
  constexpr int D = kHeadDim256;
  constexpr int KS = D / 32;             // k-steps of S^T = the 16-byte pieces a thread stages per step and tensor
  constexpr int DB = D / 16;             // 16-dim blocks of O^T
  constexpr int ROWB = 2 * D + 32;       // bytes of a K or V row in LDS
  constexpr int LPR = D / 8;             // threads per staged row
  constexpr int PASS = kThreads / LPR;   // rows one pass of the workgroup stages
  static_assert(PASS * KS == kKeyStep, "staging covers the step");
  static_assert(2 * kKeyStep * ROWB == kPrefill256LdsBytes, "the describe text states this");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kKeyStep * ROWB];
  unsigned char* const sk = smem;
  unsigned char* const sv = smem + kKeyStep * ROWB;

  // workgroup blockIdx.x = h slots + x: slot x of KV head h. The sequence and the tile of a slot: seq_of_slot_anyg (workgroup-uniform, scalar loads)
  fa2d::Split sp;
  sp.h = blockIdx.x / slots;
  const unsigned slot = blockIdx.x - sp.h * slots;
  int c0, T;
  const int bs = fa2pp::seq_of_slot_anyg(cu_q, B, total_q, G, slot, c0, T);
  if (bs < 0) return;  // a slot in front of the first sequence
  sp.b = (unsigned)bs, sp.bh = sp.b * (unsigned)kv.Hkv + sp.h, sp.s = 0, sp.lo = 0;
  const int R = T * G, Hq = kv.Hkv * G;
  const unsigned tile = slot - fa2pp::slot_of_anyg(c0, G, bs);
  if (tile >= (unsigned)((R + kRowTile - 1) / kRowTile)) return;               // a slot behind the sequence's last tile (T = 0: every one)
  const int len = min(max(seqlens[sp.b], 0), kv.nmax());
  const int row0 = (int)tile * kRowTile;                                        // < R
  const int rows = min(kRowTile, R - row0);
  const int n_end = len - (T - 1 - tok_of(row0 + rows - 1, G));                 // the keys the tile's last token sees
  const size_t row_bt = (size_t)c0 * Hq + (size_t)sp.h * G;                     // packed output row of (t, g): row_bt + t Hq + g

  if (n_end <= 0) {  // no row of the tile sees a key
    for (int idx = threadIdx.x; idx < rows * LPR; idx += kThreads) {
      const int r = row0 + idx / LPR, t = tok_of(r, G);
      const size_t row = row_bt + (size_t)t * Hq + (r - t * G);
      *reinterpret_cast<b8*>(o + row * D + 8 * (idx % LPR)) = b8{};
      if (lse && idx % LPR == 0) lse[row] = FA2D_NEG_INF;
    }
    return;
  }
  const unsigned n = (unsigned)n_end;
  // the first step any row of the tile needs: the one that holds the lower edge of its first token; < n, as that token's edge is below its keys
  const unsigned k_begin = (unsigned)window_edge(len - (T - 1 - tok_of(row0, G)), W) & ~(unsigned)(kKeyStep - 1);

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i16 = lane & 15, g4 = lane >> 4;
  const int wr0 = row0 + w * kWaveRows;  // the wave's first row; wave-uniform from here on
  const int n_wave = wr0 < R ? len - (T - 1 - tok_of(min(wr0 + kWaveRows, R) - 1, G)) : 0;  // the keys its last token sees
  const int lo_wave = wr0 < R ? window_edge(len - (T - 1 - tok_of(wr0, G)), W) : 0;         // the lower edge of its first token

  // the query fragments, the keys each lane's query sees (lo_q <= key < nq), and per row tile the keys its first token sees (0 for a tile with
  // rows >= R: those always take the select) and the lower edge of its last
  b8 qf[kMT][KS];
  unsigned nq[kMT], lo_q[kMT], n_tile[kMT], lo_tile[kMT];
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    const int rf = wr0 + 16 * qb, r = rf + i16;
    const int t = tok_of(r, G), g = r - t * G;
    nq[qb] = r < R ? (unsigned)max(len - (T - 1 - t), 0) : 0u;
    lo_q[qb] = (unsigned)window_edge((int)nq[qb], W);
    n_tile[qb] = rf + 16 <= R ? (unsigned)max(len - (T - 1 - tok_of(rf, G)), 0) : 0u;
    lo_tile[qb] = rf + 16 <= R ? (unsigned)window_edge(len - (T - 1 - tok_of(rf + 15, G)), W) : 0u;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      b8 x = {};
      if (r < R) x = *reinterpret_cast<const b8*>(q + (row_bt + (size_t)t * Hq + g) * D + 32 * ks + 8 * g4);
      qf[qb][ks] = x;
    }
  }

  // staging: this thread's column 8 (tid % LPR) .. + 7 of the rows tid / LPR + PASS i of a step
  const int s_row = threadIdx.x / LPR, s_col = threadIdx.x % LPR;
  const PagedKV::At at = kv.at(sp, D, 8 * s_col);
  const SoftCapMul cm = {scale_log2, pre, cap2};  // CAP only
  struct Rows {
    b8 k[KS], v[KS];
  };
  auto lookup = [&](int (&pg)[KS], unsigned k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) pg[i] = kv.lookup(at, k0 + s_row + PASS * i, n);
  };
  auto load = [&](Rows& d, const int (&pg)[KS], unsigned k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const unsigned r = k0 + s_row + PASS * i;
      d.k[i] = b8{}, d.v[i] = b8{};
      if (r < n) {
        const size_t e = kv.elem(at, pg[i], r, D);
        d.k[i] = *reinterpret_cast<const b8*>(at.k + e);
        d.v[i] = *reinterpret_cast<const b8*>(at.v + e);
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
  lookup(pg, k_begin);
  load(cur, pg, k_begin);
  lookup(pg, k_begin + kKeyStep);
  for (unsigned k0 = k_begin; k0 < n; k0 += kKeyStep) {
    __syncthreads();  // every wave has read the step before
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      *reinterpret_cast<b8*>(sk + s_off + PASS * i * ROWB) = cur.k[i];
      *reinterpret_cast<b8*>(sv + s_off + PASS * i * ROWB) = cur.v[i];
    }
    __syncthreads();
    Rows nxt;
    load(nxt, pg, k0 + kKeyStep);  // behind the last step every predicate is false: zeros, no access
    lookup(pg, k0 + 2 * kKeyStep);
    if ((int)k0 < n_wave && (int)(k0 + kKeyStep) > lo_wave) {  // wave-uniform: the step holds a key some row of the wave sees
      f4 st[kMT][kKB];
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb) {
        b8 kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const b8*>(k_ld + 16 * kb * ROWB + 64 * ks);
#pragma unroll
        for (int qb = 0; qb < kMT; ++qb) {
          st[qb][kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) st[qb][kb] = mfma(kf[ks], qf[qb][ks], st[qb][kb]);
        }
      }
      b8 pf[kMT][2];
#pragma unroll
      for (int qb = 0; qb < kMT; ++qb) {
        float alpha;
        // wave-uniform: every key of the step is inside the window of every row of the tile -- at or above the lower edge of its last row and
        // below the causal edge of its first
        const bool inside = k0 >= lo_tile[qb] && k0 + kKeyStep <= n_tile[qb];
        if constexpr (CAP) {
          if (inside)
            softmax_step_window_cap<false>(st[qb], k0 + 4 * g4, lo_q[qb], nq[qb], cm, m[qb], l[qb], alpha, pf[qb]);
          else
            softmax_step_window_cap<true>(st[qb], k0 + 4 * g4, lo_q[qb], nq[qb], cm, m[qb], l[qb], alpha, pf[qb]);
        } else {
          if (inside)
            softmax_step_window<false>(st[qb], k0 + 4 * g4, lo_q[qb], nq[qb], scale_log2, m[qb], l[qb], alpha, pf[qb]);
          else
            softmax_step_window<true>(st[qb], k0 + 4 * g4, lo_q[qb], nq[qb], scale_log2, m[qb], l[qb], alpha, pf[qb]);
        }
#pragma unroll
        for (int db = 0; db < DB; ++db) acc[qb][db] *= alpha;
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const unsigned char* a = v_ld + 32 * c * ROWB + 32 * db;
          const b8 vf = b8_cat(lds_read_tr(a), lds_read_tr(a + 16 * ROWB));
#pragma unroll
          for (int qb = 0; qb < kMT; ++qb) acc[qb][db] = mfma(vf, pf[qb][c], acc[qb][db]);
        }
    }
    cur = nxt;
  }

  // the row sums of the four lanes of a query, in a fixed order (both partners of a swap add the same pair); lane (g4, i16) holds dims
  // 16 db + 4 g4 .. + 3 of query i16. Then the sink of the row's head sp.h G + g, if there are sinks, joins the finished row (fold_sink), once.
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    float a, c;
    fa2d::swap_pair<16>(l[qb], a, c);
    l[qb] = a + c;
    fa2d::swap_pair<32>(l[qb], a, c);
    l[qb] = a + c;
    const int r = wr0 + 16 * qb + i16;
    if (r < R) {
      const int t = tok_of(r, G), g = r - t * G;
      const size_t row = row_bt + (size_t)t * Hq + g;
      const float f = fold_sink(m[qb], l[qb], sink_log2_or_none(sinks, sp.h * G + g));
      const float inv = l[qb] > 0.0f ? 1.0f / l[qb] : 0.0f;  // no visible key: O = 0, LSE = -inf
#pragma unroll
      for (int db = 0; db < DB; ++db) *reinterpret_cast<b4*>(o + row * D + 16 * db + 4 * g4) = round4(acc[qb][db] * f * inv);
      if (lse && g4 == 0) lse[row] = l[qb] > 0.0f ? (m[qb] + __builtin_log2f(l[qb])) * 0.6931471805599453f : FA2D_NEG_INF;
    }
  }
}

template <bool CAP>
int launch_prefill_paged_varlen_window_sink_softcap_anyg_d256(const void* q, const PagedKV& kv, const int* seqlens, const int* cu_q,
                                                              const float* sinks, void* o, float* lse, int B, int total_q, int G, long long slots,
                                                              int W, float mult, float pre, float cap2, hipStream_t stream) {
  CLN_LAUNCH((fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16_mfma<CAP>), dim3((unsigned)((long long)kv.Hkv * slots)), dim3(kThreads), 0,
             stream, (const bf16_t*)q, kv, seqlens, cu_q, sinks, (bf16_t*)o, lse, B, total_q, G, (unsigned)slots, W, mult, pre, cap2);
  return cln_check_launch();
}

}  // namespace fa2b
