// Multi-head latent attention (MLA) PREFILL for a packed batch in bf16 (cln_fa2_prefill_varlen_mla_bf16, include/cln_amd_ext.h; DESIGN
// 4.4.18): the un-absorbed form DeepSeek-V2 / V3 / R1 and Kimi-K2 run over a prompt, after kv_b_proj has up-projected the latent rows. Per
// head the key has 192 dims, [k_nope (128) | k_pe (64)], and the value 128; Hkv = Hq. Nothing is paged here.
//   q     bf16 [total_q, Hq, 192] = [q_nope 128 | q_pe 64], rotated
//   kv    bf16 [total_k, Hq, 256] = [k_nope 128 | v 128] per head: what kv_b_proj writes, no split or concat copy
//   k_pe  bf16 [total_k, 64], rotated, ONE row per token shared by every head: never broadcast in memory, every head's workgroup reads the
//         same 128 bytes
//   o     bf16 [total_q, Hq, 128], lse fp32 [total_q, Hq]
// Sequence b has T_b = cu_q[b + 1] - cu_q[b] queries and L_b = cu_k[b + 1] - cu_k[b] keys (every offset clamped, lengths max(., 0)); query t
// sees the keys j < L_b - (T_b - 1 - t) (causal, the family's bottom-right rule with len = L_b) or all L_b (causal = 0: a context chunk of a
// chunked prefill). A query that sees no key: O = 0, LSE = -inf.
//
// A SIBLING body of fa2b::fa2_prefill_paged_varlen_bf16_mfma<128> (flash_attn_prefill_paged_varlen_bf16.cuh) in a namespace of its own. Shared
// by inclusion, not repeated: the tile constants, slot_of / seq_of_slot at g_shift = 0 (slots = total_q / 128 + B per head, grid Hq slots in
// x), b8 / mfma / lds_read_tr / round4, swap_pair / ex2, and fa2b::softmax_step. The geometry is that kernel's: four waves, a 128-row tile with
// 32 rows per wave (kMT = 2), a 64-key step, the next step's rows waiting in registers over the two barriers. What differs:
//   S^T = K Q^T   6 k-steps of 32 dims, 4 from k_nope and 2 from k_pe: 4 x 6 x 2 = 48 MFMAs per wave and step (32 there)
//   O^T = V^T P^T unchanged: 8 dim blocks, 32 MFMAs; 80 per step in all (64 there)
//   staging       per thread and step 4 pieces of k_nope (16 threads per row, 16 rows per pass), 2 of k_pe (8 threads per row, 32 rows per
//                 pass), 4 of V; plain addresses: token cu_k[b] + j, head h, K at kv + (tok Hq + h) 256, V 128 elements further, k_pe + tok 64
//   LDS           K rows of 2 x 192 + 32 = 416 bytes (13 x 32), V rows of 288 (9 x 32): odd multiples of 32 as the siblings' strides;
//                 64 x 416 + 64 x 288 = 45056 bytes static
// Rows at or past the visible length are stored to LDS as zeros and not loaded. Registers: DESIGN 4.4.18 has the compiled numbers.
#pragma once
#include "flash_attn_prefill_paged_varlen_bf16.cuh"

namespace fa2mp {

using fa2b::b8_cat;
using fa2b::kThreads;
using fa2b::lds_read_tr;
using fa2b::mfma;
using fa2b::round4;
using fa2pp::kKB;
using fa2pp::kKeyStep;
using fa2pp::kMT;
using fa2pp::kRowTile;
using fa2pp::kWaveRows;

constexpr int kDn = 128, kDr = 64, kDk = kDn + kDr, kDv = 128;  // nope dims, rotary dims, key dims, value dims
constexpr int kKvRow = kDn + kDv;                               // elements of a (token, head) row of kv
constexpr int kKRowB = 2 * kDk + 32, kVRowB = 2 * kDv + 32;     // bytes of a K / V row in LDS
constexpr int kLdsBytes = kKeyStep * (kKRowB + kVRowB);
constexpr int kMfmasPerStep = kKB * (kDk / 32) * kMT + 2 * (kDv / 16) * kMT;  // 48 + 32
static_assert(kKRowB % 64 == 32 && kVRowB % 64 == 32 && kLdsBytes == 45056 && kMfmasPerStep == 80, "the layout DESIGN 4.4.18 describes");

struct Args {
  const bf16_t *q, *kv, *k_pe;
  const int *cu_q, *cu_k;
  bf16_t* o;
  float* lse;
  int B, total_q, total_k, Hq, causal;
  unsigned slots;
  float scale_log2;
};

__global__ __launch_bounds__(kThreads, 2) void fa2_prefill_varlen_mla_bf16_mfma(const Args a) {
  constexpr int KSN = kDn / 32, KSR = kDr / 32, KS = KSN + KSR;  // k-steps of S^T: 4 from k_nope, 2 from k_pe
  constexpr int DB = kDv / 16;                                   // 16-dim blocks of O^T
  constexpr int LPR = kDn / 8, PASS = kThreads / LPR;            // k_nope and V: threads per staged row, rows per pass
  constexpr int LPR_R = kDr / 8, PASS_R = kThreads / LPR_R;      // k_pe
  static_assert(PASS * KSN == kKeyStep && PASS_R * KSR == kKeyStep, "staging covers the step");
  __shared__ __attribute__((aligned(16))) unsigned char smem[kLdsBytes];
  unsigned char* const sk = smem;
  unsigned char* const sv = smem + kKeyStep * kKRowB;

  // workgroup blockIdx.x = h slots + x: slot x of head h. The sequence and the tile of a slot: seq_of_slot (workgroup-uniform, scalar loads)
  const unsigned h = blockIdx.x / a.slots;
  const unsigned slot = blockIdx.x - h * a.slots;
  int c0, T;
  const int bs = fa2pp::seq_of_slot(a.cu_q, a.B, a.total_q, 0, slot, c0, T);
  if (bs < 0) return;  // a slot in front of the first sequence
  const unsigned tile = slot - fa2pp::slot_of(c0, 0, bs);
  if (tile >= (unsigned)((T + kRowTile - 1) / kRowTile)) return;  // a slot behind the sequence's last tile (T = 0: every one)
  const int kc0 = __builtin_amdgcn_readfirstlane(min(max(a.cu_k[bs], 0), a.total_k));
  const int len = __builtin_amdgcn_readfirstlane(max(min(max(a.cu_k[bs + 1], 0), a.total_k) - kc0, 0));
  const int Hq = a.Hq, cz = a.causal ? 1 : 0;   // query t sees len - cz (T - 1 - t) keys
  const int row0 = (int)tile * kRowTile;        // < T
  const int rows = min(kRowTile, T - row0);
  const int n_end = len - cz * (T - 1 - (row0 + rows - 1));  // the keys the tile's last token sees
  const size_t row_bt = (size_t)c0 * Hq + h;                 // packed output row of token t: row_bt + t Hq
  bf16_t* const o = a.o;
  float* const lse = a.lse;

  if (n_end <= 0) {  // no row of the tile sees a key
    for (int idx = threadIdx.x; idx < rows * LPR; idx += kThreads) {
      const size_t row = row_bt + (size_t)(row0 + idx / LPR) * Hq;
      *reinterpret_cast<b8*>(o + row * kDv + 8 * (idx % LPR)) = b8{};
      if (lse && idx % LPR == 0) lse[row] = FA2D_NEG_INF;
    }
    return;
  }
  const unsigned n = (unsigned)n_end;  // <= len

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i16 = lane & 15, g4 = lane >> 4;
  const int wr0 = row0 + w * kWaveRows;  // the wave's first row; wave-uniform from here on
  const int n_wave = wr0 < T ? len - cz * (T - 1 - (min(wr0 + kWaveRows, T) - 1)) : 0;  // the keys its last token sees

  // the query fragments, the keys each lane's query sees, and per row tile the keys its first token sees (0 for a tile with rows >= T: those
  // always take the select)
  b8 qf[kMT][KS];
  unsigned nq[kMT], n_tile[kMT];
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    const int rf = wr0 + 16 * qb, r = rf + i16;
    nq[qb] = r < T ? (unsigned)max(len - cz * (T - 1 - r), 0) : 0u;
    n_tile[qb] = rf + 16 <= T ? (unsigned)max(len - cz * (T - 1 - rf), 0) : 0u;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      b8 x = {};
      if (r < T) x = *reinterpret_cast<const b8*>(a.q + (row_bt + (size_t)r * Hq) * kDk + 32 * ks + 8 * g4);
      qf[qb][ks] = x;
    }
  }

  // staging: this thread's column 8 (tid % LPR) .. + 7 of the rows tid / LPR + PASS i of k_nope and V, and column 8 (tid % LPR_R) .. + 7 of
  // the rows tid / LPR_R + PASS_R i of k_pe
  const int s_row = threadIdx.x / LPR, s_col = threadIdx.x % LPR;
  const int p_row = threadIdx.x / LPR_R, p_col = threadIdx.x % LPR_R;
  const bf16_t* const kv_at = a.kv + ((size_t)kc0 * Hq + h) * kKvRow + 8 * s_col;  // + j Hq kKvRow: key j of the sequence
  const bf16_t* const pe_at = a.k_pe + (size_t)kc0 * kDr + 8 * p_col;             // + j kDr
  struct Rows {
    b8 k[KSN], v[KSN], p[KSR];
  };
  auto load = [&](Rows& d, unsigned k0) {
#pragma unroll
    for (int i = 0; i < KSN; ++i) {
      const unsigned r = k0 + s_row + PASS * i;
      d.k[i] = b8{}, d.v[i] = b8{};
      if (r < n) {
        const bf16_t* e = kv_at + (size_t)r * Hq * kKvRow;
        d.k[i] = *reinterpret_cast<const b8*>(e);
        d.v[i] = *reinterpret_cast<const b8*>(e + kDn);
      }
    }
#pragma unroll
    for (int i = 0; i < KSR; ++i) {
      const unsigned r = k0 + p_row + PASS_R * i;
      d.p[i] = b8{};
      if (r < n) d.p[i] = *reinterpret_cast<const b8*>(pe_at + (size_t)r * kDr);
    }
  };
  const int sk_off = s_row * kKRowB + 16 * s_col;                                      // + PASS i rows
  const int sp_off = p_row * kKRowB + 2 * kDn + 16 * p_col;                            // + PASS_R i rows
  const int sv_off = s_row * kVRowB + 16 * s_col;                                      // + PASS i rows
  const unsigned char* k_ld = sk + i16 * kKRowB + 16 * g4;                             // + 16 kb rows, + 64 ks bytes
  const unsigned char* v_ld = sv + (4 * g4 + (i16 >> 2)) * kVRowB + 8 * (i16 & 3);     // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m[kMT], l[kMT];
  f4 acc[kMT][DB];
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    m[qb] = FA2D_NEG_INF, l[qb] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[qb][db] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  Rows cur;
  load(cur, 0);
  for (unsigned k0 = 0; k0 < n; k0 += kKeyStep) {
    __syncthreads();  // every wave has read the step before
#pragma unroll
    for (int i = 0; i < KSN; ++i) {
      *reinterpret_cast<b8*>(sk + sk_off + PASS * i * kKRowB) = cur.k[i];
      *reinterpret_cast<b8*>(sv + sv_off + PASS * i * kVRowB) = cur.v[i];
    }
#pragma unroll
    for (int i = 0; i < KSR; ++i) *reinterpret_cast<b8*>(sk + sp_off + PASS_R * i * kKRowB) = cur.p[i];
    __syncthreads();
    Rows nxt;
    load(nxt, k0 + kKeyStep);  // behind the last step every predicate is false: zeros, no access
    if ((int)k0 < n_wave) {    // wave-uniform
      f4 st[kMT][kKB];
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb) {
        // the four k_nope k-steps, then the two k_pe ones: at most four K fragments are alive
        b8 kf[KSN];
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) kf[ks] = *reinterpret_cast<const b8*>(k_ld + 16 * kb * kKRowB + 64 * ks);
#pragma unroll
        for (int qb = 0; qb < kMT; ++qb) {
          st[qb][kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < KSN; ++ks) st[qb][kb] = mfma(kf[ks], qf[qb][ks], st[qb][kb]);
        }
        b8 kr[KSR];
#pragma unroll
        for (int ks = 0; ks < KSR; ++ks) kr[ks] = *reinterpret_cast<const b8*>(k_ld + 16 * kb * kKRowB + 64 * (KSN + ks));
#pragma unroll
        for (int qb = 0; qb < kMT; ++qb)
#pragma unroll
          for (int ks = 0; ks < KSR; ++ks) st[qb][kb] = mfma(kr[ks], qf[qb][KSN + ks], st[qb][kb]);
      }
      b8 pf[kMT][2];
#pragma unroll
      for (int qb = 0; qb < kMT; ++qb) {
        float alpha;
        if (k0 + kKeyStep <= n_tile[qb])  // wave-uniform: every key of the step is visible to every row of the tile
          fa2b::softmax_step<false>(st[qb], k0 + 4 * g4, nq[qb], a.scale_log2, m[qb], l[qb], alpha, pf[qb]);
        else
          fa2b::softmax_step<true>(st[qb], k0 + 4 * g4, nq[qb], a.scale_log2, m[qb], l[qb], alpha, pf[qb]);
#pragma unroll
        for (int db = 0; db < DB; ++db) acc[qb][db] *= alpha;
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const unsigned char* p = v_ld + 32 * c * kVRowB + 32 * db;
          const b8 vf = b8_cat(lds_read_tr(p), lds_read_tr(p + 16 * kVRowB));
#pragma unroll
          for (int qb = 0; qb < kMT; ++qb) acc[qb][db] = mfma(vf, pf[qb][c], acc[qb][db]);
        }
    }
    cur = nxt;
  }

  // the row sums of the four lanes of a query, in a fixed order (both partners of a swap add the same pair); lane (g4, i16) holds dims
  // 16 db + 4 g4 .. + 3 of query i16
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    float x, y;
    fa2d::swap_pair<16>(l[qb], x, y);
    l[qb] = x + y;
    fa2d::swap_pair<32>(l[qb], x, y);
    l[qb] = x + y;
    const int r = wr0 + 16 * qb + i16;
    if (r < T) {
      const size_t row = row_bt + (size_t)r * Hq;
      const float inv = l[qb] > 0.0f ? 1.0f / l[qb] : 0.0f;  // no visible key: O = 0, LSE = -inf
#pragma unroll
      for (int db = 0; db < DB; ++db) *reinterpret_cast<b4*>(o + row * kDv + 16 * db + 4 * g4) = round4(acc[qb][db] * inv);
      if (lse && g4 == 0) lse[row] = l[qb] > 0.0f ? (m[qb] + __builtin_log2f(l[qb])) * 0.6931471805599453f : FA2D_NEG_INF;
    }
  }
}

// slots workgroups per head, all in x (the caller checks that the grid fits). No host read of the offsets, no allocation.
inline int launch_prefill_varlen_mla(const Args& a, hipStream_t stream) {
  CLN_LAUNCH(fa2_prefill_varlen_mla_bf16_mfma, dim3((unsigned)((long long)a.Hq * a.slots)), dim3(kThreads), 0, stream, a);
  return cln_check_launch();
}

}  // namespace fa2mp
