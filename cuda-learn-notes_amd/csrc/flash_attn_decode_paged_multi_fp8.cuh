// Multi-token ("speculative verify" / short append) decode attention over a PAGED KV cache held in FP8 (OCP e4m3fn) with one fp32 scale per KV
// head: flash_attn_decode_paged_multi.cuh with the e4m3 row source,
//   O[b,t,h,:] = sum_{j < n(b,t)} softmax_j(q[b,t,h] . (k8_j k_scale[h / G]) / sqrt(D)) (v8_j v_scale[h / G]),   n(b,t) = len_b - (T - 1 - t).
// k_pages / v_pages e4m3fn [P,Hkv,page,D], k_scale / v_scale fp32 [Hkv] on the device; everything else as there, the 128-key step, the split plan,
// the workspace layout and fa2d::fa2_decode_combine_kernel included. The kernel is a SIBLING of fa2pm::fa2_decode_paged_multi_kernel -- its body with
// the row stage changed; one body with the row source as a policy was built first and cost the fp16 kernel up to 6 % at two row tiles (DESIGN
// 4.4.6), so the fp16 source stays as it was: lane (g4, i16)
// loads 16 BYTES of key i16 per piece -- elements 64 i + 16 g4 .. + 15, so four lanes cover 64 consecutive bytes and a row of D = 64 is one load
// per lane and tensor -- and its two 8-byte halves are the lane's k-slots of the k-steps 2 i and 2 i + 1 of S^T; the query fragments are loaded
// from the same dims. The bytes wait in registers while the step before is computed and become halves once (fa2d::e4m3x8_to_h8): the K
// fragments in front of the MT row tiles, the V rows on their way into the wave's LDS image, which has the layout of the fp16 kernel. Both
// products and the softmax run on the unscaled codes; k_scale[h] multiplies the score multiplier once per workgroup, v_scale[h] the workgroup's
// O partial in front of store_split (it is linear in V), as fa2d::fa2_decode_fp8_stream does.
//
// The kernel's name does not end in _kernel: tests/decode_kernels.py labels every fa2pm::*_kernel symbol of the library by the fp16 describe
// texts.
#pragma once
#include "flash_attn_decode_paged_multi.cuh"
#include "flash_attn_paged_fp8_rows.cuh"

namespace fa2pm {

// The geometry of the e4m3 rows: a lane loads kLoads pieces of kPiece bytes of a row (lane (g4, i16), piece i: elements kPiece (4 i + g4) ..
// + kPiece - 1 of key i16); dim(ks, g4) = the first of the 8 row elements that are the lane's k-slots of k-step ks of S^T (the query fragments
// follow it: any assignment serves a dot product); halves(): those 8 elements of the loaded pieces as fp16.
template <int D>
struct RowsE4M3 {
  static constexpr int kPiece = 16, kLoads = D / 64;
  static __device__ __forceinline__ int dim(int ks, int g4) { return 64 * (ks >> 1) + 16 * g4 + 8 * (ks & 1); }
  static __device__ __forceinline__ h8 halves(const uint4 (&r)[kLoads], int ks) {
    const uint4 x = r[ks >> 1];
    return fa2d::e4m3x8_to_h8((ks & 1) ? uint2{x.z, x.w} : uint2{x.x, x.y});
  }
};

template <int D, int MT>
__global__ __launch_bounds__(kThreads) void fa2_decode_paged_multi_fp8_mfma(const half_t* __restrict__ q, const fa2d::PagedKV8 kv,
                                                                            const int* __restrict__ seqlens, const fa2d::Out out, int T,
                                                                            int g_shift, int S, int C, float scale_log2) {
  using Geo = RowsE4M3<D>;
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
  constexpr int NL = Geo::kLoads;
  const fa2d::PagedKV8::At at = kv.at(sp, Geo::kPiece * g4);
  scale_log2 *= kv.k_scale[sp.h];  // the scale of the stored K codes goes into the score multiplier, once per workgroup
  const float v_mul = kv.v_scale[sp.h];
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
      if (r < R) x = *reinterpret_cast<const h8*>(q + (row_bt + (size_t)t * Hq + g) * D + Geo::dim(ks, g4));
      qf[qb][ks] = x;
    }
  }

  const unsigned row0 = (unsigned)(w * kWaveKeys + i16);  // this lane's first row of a step; its second is 16 further
  struct Rows {
    uint4 k[2][NL], v[2][NL];
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
      for (int i = 0; i < NL; ++i) d.k[kb][i] = uint4{0u, 0u, 0u, 0u}, d.v[kb][i] = uint4{0u, 0u, 0u, 0u};
      if (r < n) {
        const size_t e = kv.elem(at, pg[kb], r, D);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          d.k[kb][i] = *reinterpret_cast<const uint4*>(at.k + e + 4 * Geo::kPiece * i);
          d.v[kb][i] = *reinterpret_cast<const uint4*>(at.v + e + 4 * Geo::kPiece * i);
        }
      }
    }
  };

  unsigned char* vw = smem + w * kWaveKeys * VROW;                      // this wave's V image: [32 rows][VROW]
  unsigned char* v_st = vw + i16 * VROW;                                 // row i16 (+ 16 kb rows); this lane's 16 bytes of k-step ks: + 2 dim(ks, g4)
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
      for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<h8*>(v_st + 16 * kb * VROW + 2 * Geo::dim(ks, g4)) = Geo::halves(cur.v[kb], ks);
    asm volatile("" ::: "memory");
    Rows nxt;
    load(nxt, pg, r0 + kKeyStep);  // behind the last step every predicate is false: zeros, no access
    lookup(pg, r0 + 2 * kKeyStep);
    const int key0 = (int)(r0 + w * kWaveKeys) + 4 * g4;  // split-local index of the key in register 0 of S^T block 0
    if (r0 + w * kWaveKeys < n) {                         // wave-uniform: EXEC stays full for the transposing reads
      h8 kf[2][KS];  // the K fragments of the step as halves: one conversion of an element, shared by the MT row tiles
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[kb][ks] = Geo::halves(cur.k[kb], ks);
#pragma unroll
      for (int qb = 0; qb < MT; ++qb) {
        f4 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          st[kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            st[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kb][ks], qf[qb][ks], st[kb], 0, 0, 0);
            cln_mfma_keep(st[kb], kf[kb][ks], qf[qb][ks]);
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
        fa2d::store_split<D>(out, row_bt + (size_t)(r >> g_shift) * Hq + (r & (G - 1)), d, sp.s, S, mx, L, O * v_mul);  // linear in V
      }
    }
    if (qb + 1 < MT) __syncthreads();
  }
}

template <int D, int MT>
int launch_decode_paged_multi_fp8(const void* q, const fa2d::PagedKV8& kv, const int* seqlens, void* o, float* lse, void* workspace, int B, int T,
                                  int g_shift, int S, int C, hipStream_t stream) {
  const long long bk = (long long)B * kv.Hkv, rows = (bk * T) << g_shift;
  const fa2d::Out out = fa2d::make_out(o, lse, workspace, rows, S, D);
  CLN_LAUNCH((fa2_decode_paged_multi_fp8_mfma<D, MT>), dim3((unsigned)(bk * S)), dim3(kThreads), 0, stream, (const half_t*)q, kv, seqlens, out, T,
             g_shift, S, C, fa2d::scale_log2(D));
  return fa2d::launch_combine<D>(cln_check_launch(), out, seqlens, rows, T * (kv.Hkv << g_shift), kv.nmax(), S, C, stream);
}

}  // namespace fa2pm
