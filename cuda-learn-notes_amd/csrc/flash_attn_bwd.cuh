// FlashAttention-2 backward, head dims 64 / 128, causal (key <= query) or not: dQ, dK, dV from Q, K, V, O, dO and the forward's
// row log-sum-exp (flash_attn_m16x_ext.hip). Two kernels on the stream, each output element summed by ONE wave in a fixed order
// (bit-repeatable; no float atomics):
//   fa2_bwd_dq_kernel    owned by a 128-row query block: writes delta = rowsum(dO o O) for its rows, then walks its key tiles
//                        (causal: up to the diagonal) -- S^T = K Q'^T, dP^T = V dO^T, dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T;
//   fa2_bwd_dkdv_kernel  owned by a 128-key block, launched behind it (reads delta): walks the query tiles (causal: from the diagonal
//                        on) -- S = Q' K^T, dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS.
// That is 7 MFMA products per (query, key) tile pair, against 5 when one kernel sums dQ with atomics.
// Both recompute the scores exactly as the forward did: the same fp16 pre-scaled Q' = Q * (log2 e / sqrt D), so P = 2^(S' - LSE log2 e)
// matches the stored LSE; the 1 / sqrt(D) of dQ and dK is applied to the fp32 sums. The row constants -LSE log2 e and -delta are the
// initial accumulators of S and dP. The accumulators of S / dP (key on the lane in the dK/dV kernel, the query in the dQ kernel) are
// packed to fp16 as the B operand of the next product; the other operand is read from ONE LDS image of the tile (rows of D halves,
// padded by 16 bytes), by rows for S and dP and by ds_read_b64_tr_b16 for the transposed products.
// 16x16x32 MFMA fragment layout (tests/test_fragment_layout_model.py): lane (i16 = lane & 15, g4 = lane >> 4) holds A[i16][8 g4 .. + 7],
// B[8 g4 .. + 7][i16]; register r of the result is C[4 g4 + r][i16].
#pragma once
#include "flash_attn_m16x.cuh"

namespace fa2b {
using fa2::GeoM16;

template <int D_>
struct BwdGeo {
  static_assert(D_ == 64 || D_ == 128, "supported head dims");
  static constexpr int D = D_, NW = 4, NT = 256;
  static constexpr int RPW = 32, BLK = NW * RPW;  // rows owned by a wave / a workgroup (queries in the dQ kernel, keys in the dK/dV kernel)
  static constexpr int TR = 64;                   // rows of a streamed tile (keys / queries)
  static constexpr int RS = D * 2 + 16;           // LDS row stride in bytes
  static constexpr int TILE = TR * RS, LDS_BYTES = 2 * TILE;
  static constexpr int NKS = D / 32, NDB = D / 16;
  static constexpr int CPR = D / 8, PF = TR * CPR / NT;  // 16-byte chunks per row; per thread and tile
};

// a tile of TR rows (row stride D halves in memory) into registers: chunk c = tid + NT i, row c / CPR
template <int D>
__device__ __forceinline__ void bwd_fetch(u4 (&r)[BwdGeo<D>::PF], const half_t* src, int tid) {
  using G = BwdGeo<D>;
#pragma unroll
  for (int i = 0; i < G::PF; ++i) {
    const int c = tid + G::NT * i;
    r[i] = *reinterpret_cast<const u4*>(src + (size_t)(c / G::CPR) * D + (c % G::CPR) * 8);
  }
}

template <int D>
__device__ __forceinline__ void bwd_store(unsigned lds, const u4 (&r)[BwdGeo<D>::PF], int tid) {
  using G = BwdGeo<D>;
#pragma unroll
  for (int i = 0; i < G::PF; ++i) {
    const int c = tid + G::NT * i;
    lds_st<u4>(lds + (c / G::CPR) * G::RS + (c % G::CPR) * 16, r[i]);
  }
}

// transposed operand from an LDS tile image: lane (i16, g4) gets rows {4 g4 + e, 16 + 4 g4 + e} (e = 0..3) of column d0 + i16, the
// k-slot order of a B operand packed from two 16-row accumulators
template <int D>
__device__ __forceinline__ h8 bwd_tr(unsigned lds, int row0, int d0, int i16, int g4) {
  using G = BwdGeo<D>;
  const unsigned a = lds + (row0 + 4 * g4 + (i16 >> 2)) * G::RS + (d0 + 4 * (i16 & 3)) * 2;
  return h8_cat(lds_read_tr16_at(a), lds_read_tr16_at(a + 16 * G::RS));
}

__device__ __forceinline__ f4 bwd_mfma(const h8& a, const h8& b, const f4& c) {
  f4 d = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  cln_mfma_keep(d, a, b);  // destination disjoint from the operands (common.h)
  return d;
}

// two workgroups per CU at D = 64; at D = 128 the Q / dO fragments, dQ and the prefetched tile need more than 256 registers
template <int D_, bool CAUSAL>
__global__ __launch_bounds__(256, D_ == 64 ? 2 : 1) void fa2_bwd_dq_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
                                                            const half_t* __restrict__ O, const half_t* __restrict__ dO, const float* __restrict__ lse,
                                                            float* __restrict__ delta, half_t* __restrict__ dQ, int N, int n_blk, int n_heads,
                                                            float scale_log2e, float scale) {
  using G = BwdGeo<D_>;
  constexpr int D = G::D, NKS = G::NKS, NDB = G::NDB, RS = G::RS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, g4 = lane >> 4;
  const int head_i = blockIdx.x % n_heads;
  const int qblk = n_blk - 1 - (int)blockIdx.x / n_heads;  // causal: the blocks with the most key tiles first
  const size_t head = (size_t)head_i * N * D, hrow = (size_t)head_i * N;
  const int q0 = qblk * G::BLK + wave * G::RPW;
  const unsigned ks_lds = hgemm::lds_addr_of(smem), vs_lds = ks_lds + G::TILE;

  // lane (i16, g4) of query block qb: row q0 + 16 qb + i16, d = 32 ks + 8 g4 .. + 7. Q' exactly as the forward rounds it.
  h8 qf[2][NKS], df[2][NKS];
  float nl[2], nd[2];
  const half_t sc = (half_t)scale_log2e;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int row = q0 + 16 * qb + i16;
    const size_t off = head + (size_t)row * D + g4 * 8;
    float acc = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      qf[qb][ks] = *reinterpret_cast<const h8*>(Q + off + ks * 32) * sc;
      df[qb][ks] = *reinterpret_cast<const h8*>(dO + off + ks * 32);
      const h8 o = *reinterpret_cast<const h8*>(O + off + ks * 32);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += (float)df[qb][ks][e] * (float)o[e];
    }
    acc += __shfl_xor(acc, 16);  // (the four lanes of the row end with the same bits: each add is commutative)
    acc += __shfl_xor(acc, 32);
    if (g4 == 0) delta[hrow + row] = acc;
    nd[qb] = -acc;
    nl[qb] = -lse[hrow + row] * 1.4426950408889634f;
  }

  f4 dq[NDB][2];
#pragma unroll
  for (int b = 0; b < NDB; ++b) dq[b][0] = dq[b][1] = f4{0.f, 0.f, 0.f, 0.f};
  const int T = CAUSAL ? (qblk + 1) * (G::BLK / G::TR) : N / G::TR;
  u4 pk[G::PF], pv[G::PF];
  bwd_fetch<D>(pk, K + head, tid);
  bwd_fetch<D>(pv, V + head, tid);
  for (int j = 0; j < T; ++j) {
    bwd_store<D>(ks_lds, pk, tid);
    bwd_store<D>(vs_lds, pv, tid);
    __syncthreads();
    if (j + 1 < T) {  // the next tile in flight under this one
      bwd_fetch<D>(pk, K + head + (size_t)(j + 1) * G::TR * D, tid);
      bwd_fetch<D>(pv, V + head + (size_t)(j + 1) * G::TR * D, tid);
    }
#pragma unroll
    for (int u = 0; u < G::TR / 32; ++u) {
      const int kr0 = j * G::TR + 32 * u;
      if (CAUSAL && kr0 > q0 + G::RPW - 1) continue;  // wave-uniform: every key of the step is past every row of the wave
      // S^T, dP^T of keys kr0 + 16 kb + 4 g4 + r (register r) and query q0 + 16 qb + i16 (the lane)
      f4 s[2][2], dp[2][2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) s[kb][qb] = f4{nl[qb], nl[qb], nl[qb], nl[qb]}, dp[kb][qb] = f4{nd[qb], nd[qb], nd[qb], nd[qb]};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const unsigned ra = (32 * u + 16 * kb + i16) * RS + (4 * ks + g4) * 16;
          const h8 kf = lds_ld<h8>(ks_lds + ra), vf = lds_ld<h8>(vs_lds + ra);
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) {
            s[kb][qb] = bwd_mfma(kf, qf[qb][ks], s[kb][qb]);
            dp[kb][qb] = bwd_mfma(vf, df[qb][ks], dp[kb][qb]);
          }
        }
      const bool diag = CAUSAL && kr0 + 31 > q0;  // wave-uniform: the step holds keys past some row of the wave
      h8 ds[2];  // B operand of dQ^T: k-slot e < 4 is key kr0 + 4 g4 + e, e >= 4 key kr0 + 16 + 4 g4 + e - 4
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float x = s[kb][qb][r];
            if (diag && kr0 + 16 * kb + 4 * g4 + r > q0 + 16 * qb + i16) x = -__builtin_inff();
            ds[qb][4 * kb + r] = (half_t)(__builtin_amdgcn_exp2f(x) * dp[kb][qb][r]);
          }
#pragma unroll
      for (int b = 0; b < NDB; ++b) {
        const h8 kt = bwd_tr<D>(ks_lds, 32 * u, 16 * b, i16, g4);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) dq[b][qb] = bwd_mfma(kt, ds[qb], dq[b][qb]);
      }
    }
    __syncthreads();
  }
  // lane (i16, g4) holds dQ[q0 + 16 qb + i16][16 b + 4 g4 .. + 3]
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int b = 0; b < NDB; ++b) {
      h4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (half_t)(dq[b][qb][e] * scale);
      *reinterpret_cast<h4*>(dQ + head + (size_t)(q0 + 16 * qb + i16) * D + 16 * b + 4 * g4) = o;
    }
}

template <int D_, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void fa2_bwd_dkdv_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
                                                              const half_t* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ delta,
                                                              half_t* __restrict__ dK, half_t* __restrict__ dV, int N, int n_heads, float scale_log2e,
                                                              float scale) {
  using G = BwdGeo<D_>;
  constexpr int D = G::D, NKS = G::NKS, NDB = G::NDB, RS = G::RS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, g4 = lane >> 4;
  const int head_i = blockIdx.x % n_heads;
  const int kblk = (int)blockIdx.x / n_heads;  // causal: the blocks with the most query tiles (low keys) first
  const size_t head = (size_t)head_i * N * D, hrow = (size_t)head_i * N;
  const int k0 = kblk * G::BLK + wave * G::RPW;
  const unsigned qs_lds = hgemm::lds_addr_of(smem), os_lds = qs_lds + G::TILE;

  // K, V of the wave's keys as the B operands of S and dP: lane (i16, g4) of key block kb: key k0 + 16 kb + i16, d = 32 ks + 8 g4 .. + 7
  h8 kf[2][NKS], vf[2][NKS];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const size_t off = head + (size_t)(k0 + 16 * kb + i16) * D + 32 * ks + 8 * g4;
      kf[kb][ks] = *reinterpret_cast<const h8*>(K + off);
      vf[kb][ks] = *reinterpret_cast<const h8*>(V + off);
    }
  f4 dv[NDB][2], dk[NDB][2];
#pragma unroll
  for (int b = 0; b < NDB; ++b)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) dv[b][kb] = dk[b][kb] = f4{0.f, 0.f, 0.f, 0.f};
  const half_t sc = (half_t)scale_log2e;
  const int j0 = CAUSAL ? kblk * (G::BLK / G::TR) : 0, T = N / G::TR;
  u4 pq[G::PF], pd[G::PF];
  bwd_fetch<D>(pq, Q + head + (size_t)j0 * G::TR * D, tid);
  bwd_fetch<D>(pd, dO + head + (size_t)j0 * G::TR * D, tid);
  for (int j = j0; j < T; ++j) {
    bwd_store<D>(qs_lds, pq, tid);
    bwd_store<D>(os_lds, pd, tid);
    __syncthreads();
    if (j + 1 < T) {
      bwd_fetch<D>(pq, Q + head + (size_t)(j + 1) * G::TR * D, tid);
      bwd_fetch<D>(pd, dO + head + (size_t)(j + 1) * G::TR * D, tid);
    }
#pragma unroll
    for (int h = 0; h < G::TR / 32; ++h) {
      const int qr0 = j * G::TR + 32 * h;
      if (CAUSAL && qr0 + 31 < k0) continue;  // wave-uniform: every row of the step is before every key of the wave
      // S, dP of query qr0 + 16 qb + 4 g4 + r (register r) and key k0 + 16 kb + i16 (the lane)
      f4 s[2][2], dp[2][2];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        const f4 l4 = *reinterpret_cast<const f4*>(lse + hrow + qr0 + 16 * qb + 4 * g4);
        const f4 d4 = *reinterpret_cast<const f4*>(delta + hrow + qr0 + 16 * qb + 4 * g4);
        s[qb][0] = s[qb][1] = l4 * -1.4426950408889634f;
        dp[qb][0] = dp[qb][1] = -d4;
      }
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          const unsigned ra = (32 * h + 16 * qb + i16) * RS + (4 * ks + g4) * 16;
          const h8 qa = lds_ld<h8>(qs_lds + ra) * sc, oa = lds_ld<h8>(os_lds + ra);
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            s[qb][kb] = bwd_mfma(qa, kf[kb][ks], s[qb][kb]);
            dp[qb][kb] = bwd_mfma(oa, vf[kb][ks], dp[qb][kb]);
          }
        }
      const bool diag = CAUSAL && qr0 < k0 + 31;  // wave-uniform: the step holds rows before some key of the wave
      h8 pp[2], dsp[2];  // B operands of dV^T / dK^T: k-slot e < 4 is query qr0 + 4 g4 + e, e >= 4 query qr0 + 16 + 4 g4 + e - 4
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float x = s[qb][kb][r];
            if (diag && k0 + 16 * kb + i16 > qr0 + 16 * qb + 4 * g4 + r) x = -__builtin_inff();
            const float p = __builtin_amdgcn_exp2f(x);
            pp[kb][4 * qb + r] = (half_t)p;
            dsp[kb][4 * qb + r] = (half_t)(p * dp[qb][kb][r]);
          }
#pragma unroll
      for (int b = 0; b < NDB; ++b) {
        const h8 ot = bwd_tr<D>(os_lds, 32 * h, 16 * b, i16, g4), qt = bwd_tr<D>(qs_lds, 32 * h, 16 * b, i16, g4);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          dv[b][kb] = bwd_mfma(ot, pp[kb], dv[b][kb]);
          dk[b][kb] = bwd_mfma(qt, dsp[kb], dk[b][kb]);
        }
      }
    }
    __syncthreads();
  }
  // lane (i16, g4) holds dK / dV[k0 + 16 kb + i16][16 b + 4 g4 .. + 3]
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int b = 0; b < NDB; ++b) {
      h4 a, c;
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = (half_t)(dk[b][kb][e] * scale), c[e] = (half_t)dv[b][kb][e];
      const size_t off = head + (size_t)(k0 + 16 * kb + i16) * D + 16 * b + 4 * g4;
      *reinterpret_cast<h4*>(dK + off) = a;
      *reinterpret_cast<h4*>(dV + off) = c;
    }
}

template <int D, bool CAUSAL>
int launch_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta, void* dq, void* dk,
               void* dv, int B, int H, int N, hipStream_t stream) {
  using G = BwdGeo<D>;
  if (N % G::BLK != 0) return CLN_ERR_UNSUPPORTED;
  const float scale = 1.0f / sqrtf((float)D), scale_log2e = 1.4426950408889634f / sqrtf((float)D);
  const int n_blk = N / G::BLK;
  CLN_LAUNCH((fa2_bwd_dq_kernel<D, CAUSAL>), dim3(n_blk * B * H), dim3(G::NT), G::LDS_BYTES, stream, (const half_t*)q, (const half_t*)k,
             (const half_t*)v, (const half_t*)o, (const half_t*)dout, lse, delta, (half_t*)dq, N, n_blk, B * H, scale_log2e, scale);
  if (cln_check_launch() != CLN_OK) return CLN_ERR_LAUNCH;
  CLN_LAUNCH((fa2_bwd_dkdv_kernel<D, CAUSAL>), dim3(n_blk * B * H), dim3(G::NT), G::LDS_BYTES, stream, (const half_t*)q, (const half_t*)k,
             (const half_t*)v, (const half_t*)dout, lse, (const float*)delta, (half_t*)dk, (half_t*)dv, N, B * H, scale_log2e, scale);
  return cln_check_launch();
}

}  // namespace fa2b
