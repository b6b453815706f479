// Prefill (any T >= 1) attention over a PAGED KV cache held in FP8 (OCP e4m3fn) with one fp32 scale per KV head: flash_attn_prefill_paged.cuh
// with the e4m3 row source,
//   O[b,t,h,:] = sum_{j < n(b,t)} softmax_j(q[b,t,h] . (k8_j k_scale[h / G]) / sqrt(D)) (v8_j v_scale[h / G]),   n(b,t) = len_b - (T - 1 - t).
// k_pages / v_pages e4m3fn [P,Hkv,page,D], k_scale / v_scale fp32 [Hkv] on the device; everything else as there. The kernel is a SIBLING of
// fa2pp::fa2_prefill_paged_kernel -- its body with the staging stage changed, softmax_step and the constants shared; one body with the row
// source as a policy was built first and cost the fp16 kernel 1 - 2.5 %, so the fp16 source stays as it was: a thread keeps the fp16 geometry of the staging stage (the same 8-element column of D / 32 rows of a
// step) and so loads 8 BYTES per row and tensor; the bytes wait in registers while the step before is computed (half the staging registers of
// the fp16 kernel) and become halves once, on their way into LDS (fa2d::e4m3x8_to_h8). The LDS image, both products and the softmax are those of
// the fp16 kernel, on the unscaled codes; k_scale[h] multiplies the score multiplier once per workgroup and v_scale[h] the final 1 / l. Rows at
// or past the cut-off of a tile are not loaded and staged as zeros, as there.
//
// The kernel's name does not end in _kernel: tests/decode_kernels.py and the fp16 surface tests count the *_kernel symbols by the fp16 describe
// texts.
#pragma once
#include "flash_attn_paged_fp8_rows.cuh"
#include "flash_attn_prefill_paged.cuh"

namespace fa2pp {

template <int D>
__global__ __launch_bounds__(kThreads, 2) void fa2_prefill_paged_fp8_mfma(const half_t* __restrict__ q, const fa2d::PagedKV8 kv,
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
  const fa2d::PagedKV8::At at = kv.at(sp, 8 * s_col);
  scale_log2 *= kv.k_scale[sp.h];  // the scale of the stored K codes goes into the score multiplier, once per workgroup
  const float v_mul = kv.v_scale[sp.h];
  struct Rows {
    uint2 k[KS], v[KS];
  };
  auto lookup = [&](int (&pg)[KS], unsigned k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) pg[i] = kv.lookup(at, k0 + s_row + PASS * i, n);
  };
  auto load = [&](Rows& d, const int (&pg)[KS], unsigned k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const unsigned r = k0 + s_row + PASS * i;
      d.k[i] = uint2{0u, 0u}, d.v[i] = uint2{0u, 0u};
      if (r < n) {
        const size_t e = kv.elem(at, pg[i], r, D);
        d.k[i] = *reinterpret_cast<const uint2*>(at.k + e);
        d.v[i] = *reinterpret_cast<const uint2*>(at.v + e);
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
      *reinterpret_cast<h8*>(sk + s_off + PASS * i * ROWB) = fa2d::e4m3x8_to_h8(cur.k[i]);  // the one conversion of an element
      *reinterpret_cast<h8*>(sv + s_off + PASS * i * ROWB) = fa2d::e4m3x8_to_h8(cur.v[i]);
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
      const float inv = (l[qb] > 0.0f ? 1.0f / l[qb] : 0.0f) * v_mul;  // no visible key: O = 0, LSE = -inf
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const f4 x = acc[qb][db] * inv;
        *reinterpret_cast<h4*>(o + row * D + 16 * db + 4 * g4) = h4{(half_t)x[0], (half_t)x[1], (half_t)x[2], (half_t)x[3]};
      }
      if (lse && g4 == 0) lse[row] = l[qb] > 0.0f ? (m[qb] + __builtin_log2f(l[qb])) * 0.6931471805599453f : FA2D_NEG_INF;
    }
  }
}

template <int D>
int launch_prefill_paged_fp8(const void* q, const fa2d::PagedKV8& kv, const int* seqlens, void* o, float* lse, int B, int T, int g_shift,
                             long long tiles, hipStream_t stream) {
  CLN_LAUNCH((fa2_prefill_paged_fp8_mfma<D>), dim3((unsigned)((long long)B * kv.Hkv * tiles)), dim3(kThreads), 0, stream, (const half_t*)q, kv,
             seqlens, (half_t*)o, lse, T, g_shift, (unsigned)tiles, fa2d::scale_log2(D));
  return cln_check_launch();
}

}  // namespace fa2pp
