// Multi-token decode attention over a PAGED KV cache in bf16 at HEAD DIM 256, with a sliding window, optional attention sinks, any query-group
// size G = Hq / Hkv in 1 ... 16, a softmax scale of the caller's and optional logit soft-capping
// (cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16, include/cln_amd_ext.h): the SIBLING of
// fa2b::fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_mfma (flash_attn_decode_paged_multi_window_sink_softcap_anyg_bf16.cuh), which takes
// D = 64 and 128. T G <= 32 query rows per KV head: MT = 1 or 2 row tiles of 16.
//
// The stream loop is not the sibling's. There a lane holds two K rows and two V rows of a 32-key wave step, and the next step's beside them: at
// D = 256 that is 64 registers per tensor and step, 192 at the loop's widest point (K of this step, K and V of the next), beside 128 accumulators
// and 64 of Q fragments at MT = 2. Here a lane holds ONE row per step: a wave takes one 16-key block, the workgroup step is 4 x 16 = 64 keys
// (kKeyStep256), and the loop's widest point is 32 (K) + 32 + 32 (K, V of the next step) = 96 registers.
//   MT = 1:  96 + 64 accumulators + 32 Q + scores and addresses: inside the 256 architectural VGPRs, two waves per SIMD
//            (__launch_bounds__(256, 2); two workgroups' LDS fit a CU)
//   MT = 2:  96 + 128 + 64 = 288 + scores and addresses: past 256. __launch_bounds__(256, 1) gives a wave the unified file of 512, and the MFMA
//            accumulators take AGPRs as their C / D operand directly; nothing is spilled.
// The price of the 16-key block: the P V product is a 16x16x32 MFMA whose 32 k-slots hold 16 keys and 16 zeros (the upper half of P and of the
// V fragment is zero), so half its depth is idle. Per 64-key step a wave issues 24 MT MFMAs for 16 KB of rows, so the idle half was expected to
// hide behind the row stream; DESIGN 4.4.16 has the measured rows and what they say about that. The alternatives: K through LDS as well as V saves no register, since the rows are
// prefetched into registers either way; the sibling's loop at a 32-key wave step needs 192 + 128 + 64 registers and leaves MT = 1 at one wave
// per SIMD as well.
// LDS: the V image of a step, 4 waves x 16 rows x (2 D + 32) = 34816 bytes, shared with the final merge of the four waves' partials,
// 4 x 16 x (D + 4 + 2) x 4 = 67072 bytes, static.
// Everything behind the loop is the sibling's: the split partials, store_split, store_final_sink and both combine kernels, which launch D
// threads per output row and index by threadIdx.x < D, instantiated here at D = 256 (fa2_decode_combine_window[_sink]_bf16_rows<256>; their
// workspace layout [rows][S][D] + [rows][S][2] comes from make_out with this D). U = max(page, 64) is what the launcher hands to the kernel and
// to the combine, and what paged::multi_window_plan_anyg_d256 planned with.
#pragma once
#include "flash_attn_decode_paged_multi_window_sink_softcap_anyg_bf16.cuh"

namespace fa2b {

constexpr int kWaveKeys256 = 16;                    // keys of one wave in one step: one 16-key S^T block
constexpr int kKeyStep256 = kWaves * kWaveKeys256;  // keys per workgroup step
constexpr int kDecode256VBytes = kWaves * kWaveKeys256 * (2 * 256 + 32);
constexpr int kDecode256LdsBytes = kWaves * 16 * (256 + 4 + 2) * 4;

template <int MT, bool CAP>
__global__ __launch_bounds__(kThreads, MT == 1 ? 2 : 1) void fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_mfma(
    const bf16_t* __restrict__ q, const PagedKV kv, const int* __restrict__ seqlens, const float* __restrict__ sinks, const Out out, int T, int G,
    int S, int C, int W, int U, float scale_log2, float pre, float cap2) {
  static_assert(MT >= 1 && MT <= 2, "row tiles");
  constexpr int D = 256;
  constexpr int KS = D / 32;         // k-steps of S^T
  constexpr int DB = D / 16;         // 16-dim blocks of O^T
  constexpr int VROW = 2 * D + 32;   // bytes of a V row in LDS: the 8 rows of a 32-lane half of a transposing read fall on 8 distinct 32-byte bank groups
  constexpr int OROW = D + 4;        // floats of an O row of the final merge
  constexpr int V_BYTES = kWaves * kWaveKeys256 * VROW;
  constexpr int M_BYTES = kWaves * 16 * (OROW + 2) * 4;
  static_assert(V_BYTES == kDecode256VBytes && M_BYTES == kDecode256LdsBytes && M_BYTES > V_BYTES, "the describe text states these");
  __shared__ __attribute__((aligned(16))) unsigned char smem[M_BYTES];

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

  const unsigned row0 = (unsigned)(w * kWaveKeys256 + i16);  // this lane's row of a step
  struct Rows {
    b8 k[KS], v[KS];
  };
  // a row at or past n is not addressed at all: its K and V fragments are zero
  auto load = [&](Rows& d, int pg, unsigned r0) {
    const unsigned r = r0 + row0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) d.k[ks] = b8{}, d.v[ks] = b8{};
    if (r < n) {
      const size_t e = kv.elem(at, pg, r, D);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        d.k[ks] = *reinterpret_cast<const b8*>(at.k + e + 32 * ks);
        d.v[ks] = *reinterpret_cast<const b8*>(at.v + e + 32 * ks);
      }
    }
  };

  unsigned char* vw = smem + w * kWaveKeys256 * VROW;                    // this wave's V image: [16 rows][VROW]
  unsigned char* v_st = vw + i16 * VROW + 16 * g4;                       // where this lane puts its 16 bytes of row i16 (+ 64 ks bytes)
  const unsigned char* v_ld = vw + (4 * g4 + (i16 >> 2)) * VROW + 8 * (i16 & 3);  // transposing read: key rows 4 g4 .. + 3, dims 16 db + i16

  float m[MT], l[MT];
  f4 acc[MT][DB];
#pragma unroll
  for (int qb = 0; qb < MT; ++qb) {
    m[qb] = FA2D_NEG_INF, l[qb] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[qb][db] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  Rows cur;
  int pg = kv.lookup(at, row0, n);  // the physical page of this lane's row of the step, fetched one step ahead of the row
  load(cur, pg, 0);
  pg = kv.lookup(at, kKeyStep256 + row0, n);
  for (unsigned r0 = 0; r0 < n; r0 += kKeyStep256) {
    asm volatile("" ::: "memory");  // the transposed reads of the step before are issued: LDS runs a wave's instructions in order
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<b8*>(v_st + 64 * ks) = cur.v[ks];
    asm volatile("" ::: "memory");
    Rows nxt;
    load(nxt, pg, r0 + kKeyStep256);  // behind the last step the predicate is false: zeros, no access
    pg = kv.lookup(at, r0 + 2 * kKeyStep256 + row0, n);
    const int key0 = (int)(r0 + w * kWaveKeys256) + 4 * g4;  // split-local index of the key in register 0 of the S^T block
    if (r0 + w * kWaveKeys256 < n) {                         // wave-uniform: EXEC stays full for the transposing reads
#pragma unroll
      for (int qb = 0; qb < MT; ++qb) {
        f4 st = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) st = mfma(cur.k[ks], qf[qb][ks], st);
        float sc[4];
        float mx = FA2D_NEG_INF;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = key0 + e;
          const float s = CAP ? softcap_score(st[e], cm) : st[e] * scale_log2;
          sc[e] = (lql[qb] <= key && key < nql[qb]) ? s : FA2D_NEG_INF;
          mx = fmaxf(mx, sc[e]);
        }
        float a, c;
        fa2d::swap_pair<16>(mx, a, c);
        mx = fmaxf(a, c);
        fa2d::swap_pair<32>(mx, a, c);
        mx = fmaxf(a, c);  // the maximum over the 16 keys of the wave step, the same in the four lanes of a query
        const float mn = fmaxf(m[qb], mx);
        const float ms = mn == FA2D_NEG_INF ? 0.0f : mn;  // no visible key yet: every factor below is exp2(-inf) = 0
        const float alpha = fa2d::ex2(m[qb] - ms);
        float ps = 0.0f;
        b8 pf = {};  // k-slots 4 .. 7 of a lane: no key, P = 0
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = fa2d::ex2(sc[e] - ms);
          ps += p;
          pf[e] = (bf16_t)p;
        }
        l[qb] = l[qb] * alpha + ps;
        m[qb] = mn;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          acc[qb][db] *= alpha;
          const b8 vf = b8_cat(lds_read_tr(v_ld + 32 * db), b4{});
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

template <int MT, bool CAP>
int launch_decode_paged_multi_window_sink_softcap_anyg_d256(const void* q, const PagedKV& kv, const int* seqlens, const float* sinks, void* o,
                                                            float* lse, void* workspace, int B, int T, int G, int S, int C, int W, float mult,
                                                            float pre, float cap2, hipStream_t stream) {
  constexpr int D = 256;
  const long long bk = (long long)B * kv.Hkv, rows = bk * T * G;
  const int page = 1 << kv.page_shift, U = page > kKeyStep256 ? page : kKeyStep256;
  const Out out = make_out(o, lse, workspace, rows, S, D);
  CLN_LAUNCH((fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_mfma<MT, CAP>), dim3((unsigned)(bk * S)), dim3(kThreads), 0, stream,
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
