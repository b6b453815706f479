// Multi-token ("speculative verify" / short append) decode attention over a PAGED KV cache with grouped query heads, on the matrix cores:
//   O[b,t,h,:] = sum_{j < n(b,t)} softmax_j(q[b,t,h] . K_j / sqrt(D)) V_j,   n(b,t) = len_b - (T - 1 - t),
//   key j of sequence b and query head h = row j % page of KV head h / G in the physical page block_table[b, j / page].
// q, o fp16 [B,T,Hq,D]; k_pages / v_pages fp16 [P,Hkv,page,D]; block_table int32 [B,max_pages] and seqlens int32 [B] ON THE DEVICE (the host reads
// neither). len_b = clamp(seqlens[b], 0, max_pages page) counts the T newest tokens, whose K / V rows the caller has written. n(b,t) <= 0 gives
// O = 0 and LSE = -inf for that query.
//
// T queries x G heads are R = T G query rows per K / V row: too many for the VALU form of flash_attn_decode_paged.cuh, nothing for
// the matrix pipe. A workgroup of 4 waves serves one (sequence, KV head, split) as there; the waves split the KEYS of a 128-key step, 32 each, and
// every wave runs all MT = ceil(R / 16) row tiles (row r = t G + g; rows >= R are zero queries that see no key and are never stored):
//   S^T = K Q^T   v_mfma_f32_16x16x32_f16, A = K rows straight from global memory (lane (g4, i16): key i16, dims 32 ks + 8 g4 .. + 7, one 16-byte
//                 load), B = the query fragments, held in registers for the whole kernel. Lane (g4, i16) register r: key 4 g4 + r, query i16.
//   softmax       online, in the base-2 domain, scores masked by SELECT (key index < n(b,t) of the lane's query), one maximum per query row shared
//                 by its four lanes (two permlane swaps), the sums per lane until the end. fa2d::ex2 and the -inf guard of fa2d::merge.
//   O^T = V^T P^T the same instruction: B = P^T rounded to fp16 in the registers S^T left it in (the two 16-key blocks of a wave step are the 8
//                 k-slots of a lane: the dataflow of flash_attn_m16x, tests/test_fragment_layout_model.py), A = V^T fragments through a
//                 wave-private LDS image of the 32 V rows and ds_read_b64_tr_b16. V rows travel global -> registers (the same addresses as the K
//                 rows: one table lookup serves both) -> LDS; rows at or past len_b are NOT loaded and stored as zeros (0 x NaN = NaN in an MFMA).
// The table entries of step i + 2 are fetched while the rows of step i + 1 are in flight (fa2d::PagedKV). The LDS image belongs to one
// wave: LDS instructions of a wave execute in order, so a compiler barrier is all the write -> transposed read -> next write chain needs.
// At the end the four waves merge per row tile through LDS (which reuses the V images) in a fixed order; with S > 1 the workgroup writes
// unnormalised fp32 partials of all its R rows -- (-inf, 0, 0) for a row that saw no key of this split -- and fa2d::fa2_decode_combine_kernel
// merges the live splits ceil(len_b / C) of a row in ascending s with the -inf guard (flash_attn_decode_common.cuh, which also has the workspace
// layout: its rows are the B T Hq query rows). No atomics.
#pragma once
#include "flash_attn_decode_common.cuh"

namespace fa2pm {

using fa2d::kThreads;
using fa2d::kWaves;
constexpr int kWaveKeys = 32;                  // keys of one wave in one step: two 16-key S^T blocks = the 32 k-slots of one P V MFMA
constexpr int kKeyStep = kWaves * kWaveKeys;  // keys per workgroup step, for both head dims
constexpr int kMaxT = 8;

template <int D, int MT>
__global__ __launch_bounds__(kThreads) void fa2_decode_paged_multi_kernel(const half_t* __restrict__ q, const fa2d::PagedKV kv,
                                                                          const int* __restrict__ seqlens, const fa2d::Out out, int T, int g_shift,
                                                                          int S, int C, float scale_log2) {
  static_assert(D == 64 || D == 128, "head dim");
  static_assert(MT >= 1 && MT <= 4, "row tiles");
  constexpr int KS = D / 32;         // k-steps of S^T
  constexpr int DB = D / 16;         // 16-dim blocks of O^T
  constexpr int VROW = 2 * D + 32;   // bytes of a V row in LDS: the 8 rows of a 32-lane half of a transposing read fall on 8 distinct 32-byte bank groups
  constexpr int OROW = D + 4;        // floats of an O row of the final merge
  constexpr int V_BYTES = kWaves * kWaveKeys * VROW;
  constexpr int M_BYTES = kWaves * 16 * (OROW + 2) * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[V_BYTES > M_BYTES ? V_BYTES : M_BYTES];

  fa2d::Split sp;
  if (!fa2d::split_of(sp, seqlens, kv.heads(), kv.nmax(), S, C)) return;
  const unsigned n = sp.n;
  const int len = sp.len, lo = sp.lo;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const fa2d::PagedKV::At at = kv.at(sp, D, 8 * g4);
  const int G = 1 << g_shift, R = T << g_shift, Hq = kv.Hkv << g_shift;
  const size_t row_bt = (size_t)sp.b * T * Hq + (size_t)sp.h * G;  // output row of (t, g): row_bt + t Hq + g

  // the query fragments and, per row tile, the number of keys OF THIS SPLIT the lane's query sees (<= 0: none)
  h8 qf[MT][KS];
  int nql[MT];
#pragma unroll
  for (int qb = 0; qb < MT; ++qb) {
    const int r = 16 * qb + i16;
    const int t = r >> g_shift, g = r & (G - 1);
    nql[qb] = r < R ? len - (T - 1 - t) - lo : 0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      h8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r < R) x = *reinterpret_cast<const h8*>(q + (row_bt + (size_t)t * Hq + g) * D + 32 * ks + 8 * g4);
      qf[qb][ks] = x;
    }
  }

  const unsigned row0 = (unsigned)(w * kWaveKeys + i16);  // this lane's first row of a step; its second is 16 further
  struct Rows {
    h8 k[2][KS], v[2][KS];
  };
  // the physical pages of this lane's two rows of the step at r0
  auto lookup = [&](int (&pg)[2], unsigned r0) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) pg[kb] = kv.lookup(at, r0 + row0 + 16 * kb, n);
  };
  // rows at or past n are not addressed at all: their K and V fragments are zero
  auto load = [&](Rows& d, const int (&pg)[2], unsigned r0) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const unsigned r = r0 + row0 + 16 * kb;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) d.k[kb][ks] = h8{0, 0, 0, 0, 0, 0, 0, 0}, d.v[kb][ks] = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (r < n) {
        const size_t e = kv.elem(at, pg[kb], r, D);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          d.k[kb][ks] = *reinterpret_cast<const h8*>(at.k + e + 32 * ks);
          d.v[kb][ks] = *reinterpret_cast<const h8*>(at.v + e + 32 * ks);
        }
      }
    }
  };

  unsigned char* vw = smem + w * kWaveKeys * VROW;                      // this wave's V image: [32 rows][VROW]
  unsigned char* v_st = vw + i16 * VROW + 16 * g4;                       // where this lane puts its 16 bytes of row i16 (+ 16 kb rows, + 64 ks bytes)
  const unsigned char* v_ld = vw + (4 * g4 + (i16 >> 2)) * VROW + 8 * (i16 & 3);  // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m[MT], l[MT];
  f4 acc[MT][DB];
#pragma unroll
  for (int qb = 0; qb < MT; ++qb) {
    m[qb] = FA2D_NEG_INF, l[qb] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[qb][db] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  Rows cur;
  int pg[2];
  lookup(pg, 0);
  load(cur, pg, 0);
  lookup(pg, kKeyStep);
  for (unsigned r0 = 0; r0 < n; r0 += kKeyStep) {
    asm volatile("" ::: "memory");  // the transposed reads of the step before are issued: LDS runs a wave's instructions in order
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<h8*>(v_st + 16 * kb * VROW + 64 * ks) = cur.v[kb][ks];
    asm volatile("" ::: "memory");
    Rows nxt;
    load(nxt, pg, r0 + kKeyStep);  // behind the last step every predicate is false: zeros, no access
    lookup(pg, r0 + 2 * kKeyStep);
    const int key0 = (int)(r0 + w * kWaveKeys) + 4 * g4;  // split-local index of the key in register 0 of S^T block 0
    if (r0 + w * kWaveKeys < n) {                         // wave-uniform: EXEC stays full for the transposing reads
#pragma unroll
      for (int qb = 0; qb < MT; ++qb) {
        f4 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          st[kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            st[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.k[kb][ks], qf[qb][ks], st[kb], 0, 0, 0);
            cln_mfma_keep(st[kb], cur.k[kb][ks], qf[qb][ks]);
          }
        }
        float sc[8];
        float mx = FA2D_NEG_INF;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          sc[e] = (key0 + 16 * (e >> 2) + (e & 3) < nql[qb]) ? st[e >> 2][e & 3] * scale_log2 : FA2D_NEG_INF;
          mx = fmaxf(mx, sc[e]);
        }
        float a, c;
        fa2d::swap_pair<16>(mx, a, c);
        mx = fmaxf(a, c);
        fa2d::swap_pair<32>(mx, a, c);
        mx = fmaxf(a, c);  // the maximum over the 32 keys of the wave step, the same in the four lanes of a query
        const float mn = fmaxf(m[qb], mx);
        const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no visible key yet: every factor below is exp2(-inf) = 0
        const float alpha = fa2d::ex2(m[qb] - ms);
        float ps = 0.0f;
        h8 pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float p = fa2d::ex2(sc[e] - ms);
          ps += p;
          pf[e] = (half_t)p;
        }
        l[qb] = l[qb] * alpha + ps;
        m[qb] = mn;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          acc[qb][db] *= alpha;
          const h8 vf = h8_cat(lds_read_tr16(v_ld + 32 * db), lds_read_tr16(v_ld + 32 * db + 16 * VROW));
          acc[qb][db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, acc[qb][db], 0, 0, 0);
          cln_mfma_keep(acc[qb][db], vf, pf);
        }
      }
    }
    cur = nxt;
  }

  // the row sums of the four lanes of a query, in a fixed order (both partners of a swap add the same pair)
#pragma unroll
  for (int qb = 0; qb < MT; ++qb) {
    float a, c;
    fa2d::swap_pair<16>(l[qb], a, c);
    l[qb] = a + c;
    fa2d::swap_pair<32>(l[qb], a, c);
    l[qb] = a + c;
  }

  // the four waves, one row tile at a time, through LDS (the V images are dead)
  float* sm_o = reinterpret_cast<float*>(smem);          // [kWaves][16][OROW]
  float* sm_ml = sm_o + kWaves * 16 * OROW;              // [kWaves][16][2]
  __syncthreads();
#pragma unroll
  for (int qb = 0; qb < MT; ++qb) {
#pragma unroll
    for (int db = 0; db < DB; ++db) *reinterpret_cast<f4*>(sm_o + (w * 16 + i16) * OROW + 16 * db + 4 * g4) = acc[qb][db];
    if (g4 == 0) sm_ml[(w * 16 + i16) * 2] = m[qb], sm_ml[(w * 16 + i16) * 2 + 1] = l[qb];
    __syncthreads();
    for (int idx = threadIdx.x; idx < 16 * D; idx += kThreads) {
      const int qi = idx / D, d = idx % D;
      const int r = 16 * qb + qi;
      if (r < R) {
        float mx, L, O;
        fa2d::reduce_waves(sm_ml + qi * 2, 16 * 2, sm_o + qi * OROW + d, 16 * OROW, mx, L, O);
        fa2d::store_split<D>(out, row_bt + (size_t)(r >> g_shift) * Hq + (r & (G - 1)), d, sp.s, S, mx, L, O);
      }
    }
    if (qb + 1 < MT) __syncthreads();
  }
}

// S splits of C keys (C a multiple of max(page, kKeyStep), S C >= max_pages page > (S - 1) C: the callers check it). No host read of the table or
// the lengths, no allocation.
template <int D, int MT>
int launch_decode_paged_multi(const void* q, const fa2d::PagedKV& kv, const int* seqlens, void* o, float* lse, void* workspace, int B, int T,
                              int g_shift, int S, int C, hipStream_t stream) {
  const long long bk = (long long)B * kv.Hkv, rows = (bk * T) << g_shift;
  const fa2d::Out out = fa2d::make_out(o, lse, workspace, rows, S, D);
  CLN_LAUNCH((fa2_decode_paged_multi_kernel<D, MT>), dim3((unsigned)(bk * S)), dim3(kThreads), 0, stream, (const half_t*)q, kv, seqlens, out, T,
             g_shift, S, C, fa2d::scale_log2(D));
  return fa2d::launch_combine<D>(cln_check_launch(), out, seqlens, rows, T * (kv.Hkv << g_shift), kv.nmax(), S, C, stream);
}

}  // namespace fa2pm
