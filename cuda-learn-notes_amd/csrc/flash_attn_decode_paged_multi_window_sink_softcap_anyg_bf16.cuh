// Multi-token decode attention over a PAGED KV cache in bf16 with a SLIDING WINDOW, optional ATTENTION SINKS, any query-group size G = Hq / Hkv in
// 1 ... 16, a SOFTMAX SCALE of the caller's and optional LOGIT SOFT-CAPPING s <- cap tanh(s / cap)
// (cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16, include/cln_amd_ext.h): the SIBLING of
// fa2b::fa2_decode_paged_multi_window_sink_anyg_bf16_mfma (flash_attn_decode_paged_multi_window_sink_anyg_bf16.cuh). The body is that kernel's
// with one compile-time flag:
//   CAP = false  the sibling statement for statement; the score multiplier scale_log2 is the caller's x log2(e) in place of log2(e) / sqrt(D).
//                With the default scale the launcher passes fa2d::scale_log2(D) and the bits are the sibling's.
//   CAP = true   the score of a visible key is softcap_score (paged_softcap.cuh), cap2 tanh(q.k x / cap); a hidden key is -inf as before, not
//                -cap. Nothing behind the scores changes: the split partials, store_split, store_final_sink, both combine kernels and fold_sink
//                are the sibling's, by inclusion -- the sink is neither scaled nor capped.
// Repeated: the stream body.
#pragma once
#include "flash_attn_decode_paged_multi_window_sink_anyg_bf16.cuh"
#include "paged_softcap.cuh"

namespace fa2b {

template <int D, int MT, bool CAP>
__global__ __launch_bounds__(kThreads) void fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_mfma(
    const bf16_t* __restrict__ q, const PagedKV kv, const int* __restrict__ seqlens, const float* __restrict__ sinks, const Out out, int T, int G,
    int S, int C, int W, int U, float scale_log2, float pre, float cap2) {
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
  const SoftCapMul cm = {scale_log2, pre, cap2};  // CAP only
  const int R = T * G, Hq = kv.Hkv * G;
  const size_t row_bt = (size_t)sp.b * T * Hq + (size_t)sp.h * G;  // output row of (t, g): row_bt + t Hq + g

  // the query fragments and, per row tile, the keys OF THIS SPLIT the lane's query sees: the split-local indices lql <= key < nql (nql <= 0: none)
  b8 qf[MT][KS];
  int nql[MT], lql[MT];
#pragma unroll
  for (int qb = 0; qb < MT; ++qb) {
    const int r = 16 * qb + i16;
    const int t = tok_of(r, G), g = r - t * G;
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

  // CAP at D = 128 with four row tiles: the uncapped kernel fills the 256 VGPRs, and the tanh temporaries come on top. This instantiation keeps
  // the running (m, l) of a row tile in accumulation registers between its uses (acc_park / acc_fetch, paged_softcap.cuh): one read and one
  // write per tile and step, and nothing is spilled
  constexpr bool PARK = CAP && D == 128 && MT == 4;
  float m[MT], l[MT];
  f4 acc[MT][DB];
#pragma unroll
  for (int qb = 0; qb < MT; ++qb) {
    m[qb] = acc_park<PARK>(FA2D_NEG_INF), l[qb] = acc_park<PARK>(0.0f);
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
          const float s = CAP ? softcap_score(st[e >> 2][e & 3], cm) : st[e >> 2][e & 3] * scale_log2;
          sc[e] = (lql[qb] <= key && key < nql[qb]) ? s : FA2D_NEG_INF;
          mx = fmaxf(mx, sc[e]);
        }
        float a, c;
        fa2d::swap_pair<16>(mx, a, c);
        mx = fmaxf(a, c);
        fa2d::swap_pair<32>(mx, a, c);
        mx = fmaxf(a, c);  // the maximum over the 32 keys of the wave step, the same in the four lanes of a query
        const float m_old = acc_fetch<PARK>(m[qb]);
        const float mn = fmaxf(m_old, mx);
        const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no visible key yet: every factor below is exp2(-inf) = 0
        const float alpha = fa2d::ex2(m_old - ms);
        float ps = 0.0f;
        b8 pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float p = fa2d::ex2(sc[e] - ms);
          ps += p;
          pf[e] = (bf16_t)p;
        }
        l[qb] = acc_park<PARK>(acc_fetch<PARK>(l[qb]) * alpha + ps);
        m[qb] = acc_park<PARK>(mn);
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
    m[qb] = acc_fetch<PARK>(m[qb]), l[qb] = acc_fetch<PARK>(l[qb]);
    float a, c;
    fa2d::swap_pair<16>(l[qb], a, c);
    l[qb] = a + c;
    fa2d::swap_pair<32>(l[qb], a, c);
    l[qb] = a + c;
  }

  // the four waves, one row tile at a time, through LDS (the V images are dead). One split: the row is finished here and its head's sink, head
  // sp.h G + g of row t G + g, if there are sinks, joins it; more: the raw partial, and the combine kernel folds the sink
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
        const int t = tok_of(r, G), g = r - t * G;
        const size_t row = row_bt + (size_t)t * Hq + g;
        if (S == 1)
          store_final_sink<D>(out, row, d, mx, L, O, sink_log2_or_none(sinks, sp.h * G + g));
        else
          store_split<D>(out, row, d, sp.s, S, mx, L, O);
      }
    }
    if (qb + 1 < MT) __syncthreads();
  }
}

// launch_decode_paged_multi_window_sink_anyg with the multipliers of paged::softcap_arg; CAP = false without a cap. The combine kernels are the
// siblings', by inclusion: the cap changes nothing behind the scores
template <int D, int MT, bool CAP>
int launch_decode_paged_multi_window_sink_softcap_anyg(const void* q, const PagedKV& kv, const int* seqlens, const float* sinks, void* o, float* lse,
                                                       void* workspace, int B, int T, int G, int S, int C, int W, float mult, float pre,
                                                       float cap2, hipStream_t stream) {
  const long long bk = (long long)B * kv.Hkv, rows = bk * T * G;
  const int page = 1 << kv.page_shift, U = page > kMultiKeyStep ? page : kMultiKeyStep;
  const Out out = make_out(o, lse, workspace, rows, S, D);
  CLN_LAUNCH((fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_mfma<D, MT, CAP>), dim3((unsigned)(bk * S)), dim3(kThreads), 0, stream,
             (const bf16_t*)q, kv, seqlens, sinks, out, T, G, S, C, W, U, mult, pre, cap2);
  const int rc = cln_check_launch();
  if (rc != CLN_OK || S == 1) return rc;
  const int Hq = kv.Hkv * G;
  if (sinks)
    CLN_LAUNCH((fa2_decode_combine_window_sink_bf16_rows<D>), dim3((unsigned)rows), dim3(D), 0, stream, (const float*)out.ws_o,
               (const float*)out.ws_ml, seqlens, sinks, out.o, out.lse, T * Hq, Hq, kv.nmax(), S, C, T, W, U);
  else
    CLN_LAUNCH((fa2_decode_combine_window_bf16_rows<D>), dim3((unsigned)rows), dim3(D), 0, stream, (const float*)out.ws_o, (const float*)out.ws_ml,
               seqlens, out.o, out.lse, T * Hq, kv.nmax(), S, C, T, W, U);
  return cln_check_launch();
}

}  // namespace fa2b
