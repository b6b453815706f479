// Multi-token decode attention over a PAGED KV cache in bf16 with a SLIDING WINDOW and ATTENTION SINKS (cln_fa2_decode_paged_multi_window_sink_bf16,
// include/cln_amd_ext.h): the SIBLING of fa2b::fa2_decode_paged_multi_window_bf16_mfma (flash_attn_decode_paged_multi_window_bf16.cuh,
// which has the mask and the split arithmetic). A sink is one fp32 logit per query head, in natural-log units and NOT scaled by 1/sqrt(D), that joins
// the softmax denominator of every row of its head and carries no value:
//   O = sum_j p_j v_j / (sum_j p_j + exp(sink_h - m)),  LSE = ln(sum_j exp(s_j) + exp(sink_h)).
//
// Shared by inclusion: window_base, window_split, the step constants, Split, the plan, reduce_waves, swap_pair, ex2, the element type, Out,
// store_final. Repeated: the stream body and the combine. The key loop is the sibling's, statement for statement; the sink enters ONCE per row, at
// the final normalisation -- in the stream kernel's store when S == 1, in the combine kernel when S > 1 (the splits store their raw (m, l, O)
// partials as the sibling does, in the sibling's workspace layout) -- through fold_sink / store_final_sink below, which the prefill's epilogue
// (flash_attn_prefill_paged_varlen_window_sink_bf16.cuh) uses too.
#pragma once
#include "flash_attn_decode_paged_multi_window_bf16.cuh"

namespace fa2b {

// The sink of a head in the units of m: formed once, in fp32. The empty asm keeps the product a value of its own: under -ffp-contract=fast the
// compiler otherwise folds the multiplication into the subtraction sink2 - m' of fold_sink (one fma with an unrounded product), and for a sink above
// the row's maximum that difference is then the product's rounding error, not 0 -- at 1e30 an exponent of +-1e23.
__device__ __forceinline__ float sink_log2(const float* __restrict__ sinks, unsigned head) {
  float s2 = sinks[head] * 1.4426950408889634f;
  asm volatile("" : "+v"(s2));
  return s2;
}

// The sink joins a finished row (m = its maximum in log2 units, l = its sum of exp2(s - m) over the keys): m' = max(m, sink2), l' = l f +
// exp2(sink2 - m'), and O is to be scaled by the f = exp2(m - m') returned. One of the two exponents is 0, so nothing overflows for any finite
// sink2. A row that sees no key (l = 0) stays one: f = 1, m and l untouched. sink2 = -inf, or so far below m that exp2 gives 0: f = exp2(0) = 1 and
// l' = fma(l, 1, 0) = l, the sibling's bits.
__device__ __forceinline__ float fold_sink(float& m, float& l, float sink2) {
  if (!(l > 0.0f)) return 1.0f;
  const float mn = fmaxf(m, sink2);
  const float f = fa2d::ex2(m - mn);
  l = fmaf(l, f, fa2d::ex2(sink2 - mn));  // spelled out, as in reduce_waves
  m = mn;
  return f;
}

// store_final with the sink folded in first
template <int D>
__device__ __forceinline__ void store_final_sink(const Out& out, size_t row, int t, float mx, float L, float O, float sink2) {
  const float f = fold_sink(mx, L, sink2);
  store_final<D>(out, row, t, mx, L, O * f);
}

template <int D, int MT>
__global__ __launch_bounds__(kThreads) void fa2_decode_paged_multi_window_sink_bf16_mfma(const bf16_t* __restrict__ q, const PagedKV kv,
                                                                                         const int* __restrict__ seqlens,
                                                                                         const float* __restrict__ sinks, const Out out, int T,
                                                                                         int g_shift, int S, int C, int W, int U, float scale_log2) {
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
  if (!window_split(sp, seqlens, kv.heads(), kv.nmax(), S, C, T, W, U)) return;
  const unsigned n = sp.n;
  const int len = sp.len, lo = sp.lo;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const PagedKV::At at = kv.at(sp, D, 8 * g4);
  const int G = 1 << g_shift, R = T << g_shift, Hq = kv.Hkv << g_shift;
  const size_t row_bt = (size_t)sp.b * T * Hq + (size_t)sp.h * G;  // output row of (t, g): row_bt + t Hq + g

  // the query fragments and, per row tile, the keys OF THIS SPLIT the lane's query sees: the split-local indices lql <= key < nql (nql <= 0: none)
  b8 qf[MT][KS];
  int nql[MT], lql[MT];
#pragma unroll
  for (int qb = 0; qb < MT; ++qb) {
    const int r = 16 * qb + i16;
    const int t = r >> g_shift, g = r & (G - 1);
    const int nqa = len - (T - 1 - t);  // the keys the query sees without a window; its lower edge is max(0, nqa - W)
    nql[qb] = r < R ? nqa - lo : 0;
    lql[qb] = r < R ? (nqa > W ? nqa - W : 0) - lo : 0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      b8 x = {};
      if (r < R) x = *reinterpret_cast<const b8*>(q + (row_bt + (size_t)t * Hq + g) * D + 32 * ks + 8 * g4);
      qf[qb][ks] = x;
    }
  }

  const unsigned row0 = (unsigned)(w * kWaveKeys + i16);  // this lane's first row of a step; its second is 16 further
  struct Rows {
    b8 k[2][KS], v[2][KS];
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
      for (int ks = 0; ks < KS; ++ks) d.k[kb][ks] = b8{}, d.v[kb][ks] = b8{};
      if (r < n) {
        const size_t e = kv.elem(at, pg[kb], r, D);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          d.k[kb][ks] = *reinterpret_cast<const b8*>(at.k + e + 32 * ks);
          d.v[kb][ks] = *reinterpret_cast<const b8*>(at.v + e + 32 * ks);
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
  lookup(pg, kMultiKeyStep);
  for (unsigned r0 = 0; r0 < n; r0 += kMultiKeyStep) {
    asm volatile("" ::: "memory");  // the transposed reads of the step before are issued: LDS runs a wave's instructions in order
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<b8*>(v_st + 16 * kb * VROW + 64 * ks) = cur.v[kb][ks];
    asm volatile("" ::: "memory");
    Rows nxt;
    load(nxt, pg, r0 + kMultiKeyStep);  // behind the last step every predicate is false: zeros, no access
    lookup(pg, r0 + 2 * kMultiKeyStep);
    const int key0 = (int)(r0 + w * kWaveKeys) + 4 * g4;  // split-local index of the key in register 0 of S^T block 0
    if (r0 + w * kWaveKeys < n) {                         // wave-uniform: EXEC stays full for the transposing reads
#pragma unroll
      for (int qb = 0; qb < MT; ++qb) {
        f4 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          st[kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) st[kb] = mfma(cur.k[kb][ks], qf[qb][ks], st[kb]);
        }
        float sc[8];
        float mx = FA2D_NEG_INF;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int key = key0 + 16 * (e >> 2) + (e & 3);
          sc[e] = (lql[qb] <= key && key < nql[qb]) ? st[e >> 2][e & 3] * scale_log2 : FA2D_NEG_INF;
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
        b8 pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float p = fa2d::ex2(sc[e] - ms);
          ps += p;
          pf[e] = (bf16_t)p;
        }
        l[qb] = l[qb] * alpha + ps;
        m[qb] = mn;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          acc[qb][db] *= alpha;
          const b8 vf = b8_cat(lds_read_tr(v_ld + 32 * db), lds_read_tr(v_ld + 32 * db + 16 * VROW));
          acc[qb][db] = mfma(vf, pf, acc[qb][db]);
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

  // the four waves, one row tile at a time, through LDS (the V images are dead). One split: the row is finished here and its head's sink, head
  // sp.h G + g of row t G + g, joins it; more: the raw partial, and the combine kernel folds the sink
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
        const size_t row = row_bt + (size_t)(r >> g_shift) * Hq + (r & (G - 1));
        if (S == 1)
          store_final_sink<D>(out, row, d, mx, L, O, sink_log2(sinks, sp.h * G + (r & (G - 1))));
        else
          store_split<D>(out, row, d, sp.s, S, mx, L, O);
      }
    }
    if (qb + 1 < MT) __syncthreads();
  }
}

// fa2b::fa2_decode_combine_window_bf16_rows with the sink of the row's head (row % Hq: the rows are [B][T][Hq]) folded into the merged row
template <int D>
__global__ __launch_bounds__(D) void fa2_decode_combine_window_sink_bf16_rows(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                                              const int* __restrict__ seqlens,
                                                                              const float* __restrict__ sinks, bf16_t* __restrict__ o,
                                                                              float* __restrict__ lse, int rows_per_seq, int Hq, int Nmax, int S,
                                                                              int C, int T, int W, int U) {
  const unsigned row = blockIdx.x;
  const int t = threadIdx.x;
  const int len = min(max(seqlens[row / (unsigned)rows_per_seq], 0), Nmax);
  const unsigned rest = (unsigned)(len - window_base(len, T, W, U));
  const int live = (int)((rest + (unsigned)C - 1u) / (unsigned)C);  // <= S: the sibling header's inequality
  const float* ml = ws_ml + (size_t)row * S * 2;
  const float* po = ws_o + (size_t)row * S * D + t;
  float mx = FA2D_NEG_INF;
  for (int s = 0; s < live; ++s) mx = fmaxf(mx, ml[2 * s]);
  const float ms = mx == FA2D_NEG_INF ? 0.0f : mx;  // never exp2(-inf + inf)
  float L = 0.0f, O = 0.0f;
  for (int s = 0; s < live; ++s) {
    const float f = fa2d::ex2(ml[2 * s] - ms);
    L = fmaf(ml[2 * s + 1], f, L);
    O = fmaf(po[(size_t)s * D], f, O);
  }
  store_final_sink<D>(Out{o, lse, nullptr, nullptr}, row, t, mx, L, O, sink_log2(sinks, row % (unsigned)Hq));
}

// launch_decode_paged_multi_window with the sinks [Hq]: to the stream kernel, which reads them when S == 1, and to the combine
template <int D, int MT>
int launch_decode_paged_multi_window_sink(const void* q, const PagedKV& kv, const int* seqlens, const float* sinks, void* o, float* lse,
                                          void* workspace, int B, int T, int g_shift, int S, int C, int W, hipStream_t stream) {
  const long long bk = (long long)B * kv.Hkv, rows = (bk * T) << g_shift;
  const int page = 1 << kv.page_shift, U = page > kMultiKeyStep ? page : kMultiKeyStep;
  const Out out = make_out(o, lse, workspace, rows, S, D);
  CLN_LAUNCH((fa2_decode_paged_multi_window_sink_bf16_mfma<D, MT>), dim3((unsigned)(bk * S)), dim3(kThreads), 0, stream, (const bf16_t*)q, kv,
             seqlens, sinks, out, T, g_shift, S, C, W, U, fa2d::scale_log2(D));
  const int rc = cln_check_launch();
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_combine_window_sink_bf16_rows<D>), dim3((unsigned)rows), dim3(D), 0, stream, (const float*)out.ws_o,
             (const float*)out.ws_ml, seqlens, sinks, out.o, out.lse, T * (kv.Hkv << g_shift), kv.Hkv << g_shift, kv.nmax(), S, C, T, W, U);
  return cln_check_launch();
}

}  // namespace fa2b
