// Prefill (any T >= 1) attention over a PAGED KV cache with grouped query heads, on the matrix cores: the semantics of
// flash_attn_decode_paged_multi.cuh with T unbounded,
//   O[b,t,h,:] = sum_{j < n(b,t)} softmax_j(q[b,t,h] . K_j / sqrt(D)) V_j,   n(b,t) = len_b - (T - 1 - t),
//   key j of sequence b and query head h = row j % page of KV head h / G in the physical page block_table[b, j / page].
// q, o fp16 [B,T,Hq,D]; k_pages / v_pages fp16 [P,Hkv,page,D]; block_table int32 [B,max_pages] and seqlens int32 [B] ON THE DEVICE (the host reads
// neither). len_b = clamp(seqlens[b], 0, max_pages page) counts the T newest tokens, whose K / V rows the caller has written (kv_append_paged.cuh: a
// sequence with len_b < T has its live tokens right-aligned). n(b,t) <= 0 gives O = 0 and LSE = -inf for that query.
//
// Where the multi kernel keeps all T G rows in one workgroup and splits the KEYS over its waves, this one splits the ROWS: the query rows of a
// (sequence, KV head), ordered r = t G + g as there, are cut into tiles of kRowTile = 128; a workgroup of 4 waves owns one tile, a wave 32 rows of
// it (two 16-row MFMA tiles), and the workgroup walks the keys 0 .. n(b, last token of the tile) in steps of kKeyStep = 64. One launch, no split
// over the keys, no workspace, no atomics: the summation order of a row is fixed by its position alone.
//   staging       the K and V rows of a step travel global -> registers -> LDS once per workgroup: a thread owns the same 16-byte column of
//                 D / 32 rows of the step, resolves their pages through fa2d::PagedKV (the entries of step i + 2 are fetched while the rows of
//                 step i + 1 are in flight and step i is computed), and rows at or past n(b, last token of the tile) -- so all rows >= len_b --
//                 are NOT loaded and stored as zeros (0 x NaN = NaN in an MFMA). Rows of 2 D + 32 bytes: the 16-byte reads of a K fragment and
//                 the 8 rows of a 32-lane half of a transposing read fall on distinct banks.
//   S^T = K Q^T   v_mfma_f32_16x16x32_f16, A = K rows from LDS (lane (g4, i16): key i16 of a 16-key block, dims 32 ks + 8 g4 .. + 7), shared by
//                 the wave's two row tiles, B = the query fragments, in registers for the whole kernel. Lane (g4, i16) register r: key 4 g4 + r,
//                 query i16.
//   softmax       online, base 2, fp32. Only a step that can cross the causal edge of a row of the 16-row tile (key0 + 64 > n of the tile's
//                 first row, or a tile with rows >= R) pays the SELECT key < n(b,t); the steps below it take the scores as they are.
//   O^T = V^T P^T the same instruction: B = P^T rounded to fp16 in the registers S^T left it in (two 16-key blocks = the 8 k-slots of a lane;
//                 tests/test_fragment_layout_model.py), A = V^T through ds_read_b64_tr_b16, shared by the two row tiles.
// A wave whose 32 rows all see no key of a step (wave-uniform: EXEC stays full for the transposing reads) skips its products but keeps the
// barriers; a tile whose rows all see no key at all stores zeros / -inf and returns.
#pragma once
#include "flash_attn_decode_common.cuh"

namespace fa2pp {

using fa2d::kThreads;
using fa2d::kWaves;
constexpr int kWaveRows = 32;                  // query rows of one wave: two MFMA row tiles
constexpr int kRowTile = kWaves * kWaveRows;  // query rows of a workgroup
constexpr int kKeyStep = 64;                   // keys per workgroup step: four 16-key S^T blocks = two 32-slot P V products
constexpr int kMT = kWaveRows / 16;
constexpr int kKB = kKeyStep / 16;

// One 16-row tile's online-softmax step over the 64 keys of S^T st: (m, l) updated, alpha = the factor of the old accumulators, pf = P^T in fp16
// as the B operand of the two P V products. MASK: keys at or past nq (the keys this lane's query sees) are dropped by select.
template <bool MASK>
__device__ __forceinline__ void softmax_step(const f4 (&st)[kKB], unsigned key0, unsigned nq, float scale_log2, float& m, float& l, float& alpha,
                                             h8 (&pf)[2]) {
  float sc[4 * kKB];
  float mx = FA2D_NEG_INF;
#pragma unroll
  for (int e = 0; e < 4 * kKB; ++e) {
    const float s = st[e >> 2][e & 3] * scale_log2;
    sc[e] = (!MASK || key0 + 16 * (e >> 2) + (e & 3) < nq) ? s : FA2D_NEG_INF;
    mx = fmaxf(mx, sc[e]);
  }
  float a, c;
  fa2d::swap_pair<16>(mx, a, c);
  mx = fmaxf(a, c);
  fa2d::swap_pair<32>(mx, a, c);
  mx = fmaxf(a, c);  // the maximum over the 64 keys of the step, the same in the four lanes of a query
  const float mn = fmaxf(m, mx);
  const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no visible key yet: every factor below is exp2(-inf) = 0
  alpha = fa2d::ex2(m - ms);
  float ps = 0.0f;
#pragma unroll
  for (int e = 0; e < 4 * kKB; ++e) {
    const float p = fa2d::ex2(sc[e] - ms);
    ps += p;
    pf[e >> 3][e & 7] = (half_t)p;
  }
  l = l * alpha + ps;
  m = mn;
}

template <int D>
__global__ __launch_bounds__(kThreads, 2) void fa2_prefill_paged_kernel(const half_t* __restrict__ q, const fa2d::PagedKV kv,
                                                                        const int* __restrict__ seqlens, half_t* __restrict__ o,
                                                                        float* __restrict__ lse, int T, int g_shift, unsigned tiles,
                                                                        float scale_log2) {
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

  // workgroup blockIdx.x = (b Hkv + h) tiles + (tiles - 1 - tile): the tiles with the most keys start first
  fa2d::Split sp;
  sp.bh = blockIdx.x / tiles;
  const unsigned tile = tiles - 1u - (blockIdx.x - sp.bh * tiles);
  sp.b = sp.bh / (unsigned)kv.Hkv, sp.h = sp.bh - sp.b * (unsigned)kv.Hkv, sp.s = 0, sp.lo = 0;
  const int len = min(max(seqlens[sp.b], 0), kv.nmax());
  const int G = 1 << g_shift, R = T << g_shift, Hq = kv.Hkv << g_shift;
  const int row0 = (int)tile * kRowTile;                                        // < R
  const int rows = min(kRowTile, R - row0);
  const int n_end = len - (T - 1 - ((row0 + rows - 1) >> g_shift));             // the keys the tile's last token sees
  const size_t row_bt = (size_t)sp.b * T * Hq + (size_t)sp.h * G;               // output row of (t, g): row_bt + t Hq + g

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

// tiles = ceil(T G / kRowTile) workgroups per (sequence, KV head), all in x (the callers check that the grid fits). No host read of the table or
// the lengths, no allocation.
template <int D>
int launch_prefill_paged(const void* q, const fa2d::PagedKV& kv, const int* seqlens, void* o, float* lse, int B, int T, int g_shift,
                         long long tiles, hipStream_t stream) {
  CLN_LAUNCH((fa2_prefill_paged_kernel<D>), dim3((unsigned)((long long)B * kv.Hkv * tiles)), dim3(kThreads), 0, stream, (const half_t*)q, kv,
             seqlens, (half_t*)o, lse, T, g_shift, (unsigned)tiles, fa2d::scale_log2(D));
  return cln_check_launch();
}

}  // namespace fa2pp
