// What the three block-scaled FP8 (OCP e4m3fn) GEMMs on the FP8 matrix pipe of gfx950 share: the dense
// form (gemm_fp8_block128.cuh), the grouped form over expert offsets (gemm_fp8_block128_grouped.cuh) and the fused gate/up form
// (gemm_fp8_block128_grouped_swiglu.cuh) include this header and nothing of one another. It owns the constants, the arithmetic of one element
// (mfma128, scale_add), the operand loads, the swizzle, and the two bodies the dense and the grouped form run: skinny<MT> and tile, whose
// first row is a parameter. It defines no kernel, no plan and no launch: each form's header defines its own, so a unit holds its own kernels
// only. The gate/up form keeps its own skinny K loop and its own ring, for the measured reason given in its header.
//   out[m, n] = bf16_rne( sum_kb  a_scale[m, kb] * b_scale[n / 128, kb] * sum_{k in block kb} fp32(a[m, k]) * fp32(b[n, k]) )
// The inner sum is ONE v_mfma_f32_16x16x128_f8f6f4 with a zero C operand, both format selectors e4m3 and no hardware scale (the hardware scale
// is e8m0 per 32 elements and cannot carry an fp32 scale); the outer sum is fp32 in ascending kb: per K block and 16 x 16 sub-tile one product
// s = sa * sb and four fmaf(s, t[i], acc[i]) into the fp32 master accumulator.
//
// ORIENTATION. The tile is computed transposed: the weight rows n are the MFMA's A operand (SrcA), the activation rows m its B operand. With
// g = lane / 16 and j = lane % 16:
//   SrcA, 8 VGPRs: the 32 bytes b[n0 + j, 128 kb + 32 g ... + 31]          (byte i of the 32 = k offset i: memory order)
//   SrcB, 8 VGPRs: the 32 bytes a[m0 + j, 128 kb + 32 g ... + 31]
//   D, 4 VGPRs:    D[r] = sum_k b[n0 + 4 g + r, k] a[m0 + j, k]: four consecutive n of ONE m
// so a_scale[m, kb] is one value per lane and K block, b_scale[n / 128, kb] is uniform over a workgroup (every strip of n lies inside one
// 128-row scale block: one scalar load per K block), and a store is four consecutive n of one m per lane and sub-tile.
// Both operands take their 32 bytes from memory by the SAME rule, so any order of the bytes inside a lane's 32 that the matrix pipe applies
// to SrcA it applies to SrcB, and the dot product does not depend on it; what the result does depend on -- lane group g holding K slice g, and
// row j in lane j of both operands -- is what the one-hot exact test at (16, 16, 128) pins (tests/test_gpu_gemm_fp8_block128.py).
//
// SKINNY (decode, weight-bandwidth-bound: N K bytes once against 2 M N K flops). A workgroup of W waves (W = 2 or 4: a strip of 32 or 64
// weight rows) owns its strip and ALL of M, padded to 16 MT rows, MT in {1, 2, 4}, row indices clamped on load and stores masked. A wave owns
// 16 weight rows. Weights go from global memory straight into the MFMA operand registers, 32 contiguous bytes a lane as two 16-byte loads,
// through a ring of kPF = 4 K blocks in registers: each weight byte is read by exactly one wave, and four blocks (2 KiB each a wave) are in
// flight under the MFMAs of the current one. The activation fragments (MT x 32 bytes a lane) and their scales (MT floats a lane) also go
// straight to registers, one K block ahead: every wave reads the whole activation tile, which is at most 64 x K bytes and stays in L2; LDS
// would save L2 reads (W-fold), not HBM reads, and is not used: no LDS, no barrier. No split over K: no workspace, no second launch.
//   Register budget, MT = 4, before the compiler: weights 4 x 8 = 32, activations 2 x 4 x 8 = 64, their scales 2 x 4 = 8, master
//   accumulators 4 x 4 = 16, one MFMA result 4, addresses ~ 16: ~ 140 VGPRs. (What hipcc reports stands in DESIGN 4.4.27.)
//
// TILE (prefill, compute-bound). Four waves, output tile 128 (m) x 128 (n); wave w owns the quarter n in [64 (w & 1), +64),
// m in [64 (w >> 1), +64): 4 x 4 sub-tiles, 64 fp32 master accumulators; per K block it holds its 4 weight fragments and streams the 4
// activation fragments. The tile's first row m_t is the caller's: 128 blockIdx.y (dense) or 128 t on the view of one expert (grouped).
// Both operands go through LDS in K blocks of 128 bytes a row, a ring of 2 slots of 128 x 128 (weights) + 128 x 128 (activations) + 128
// floats (the rows' sa of this block) = 33280 bytes; 66560 bytes static. The ring is filled THROUGH REGISTERS (four 16-byte global loads a
// thread and operand, issued in front of the block's MFMAs, written to the other slot behind them, one barrier a K block), not by LDS-DMA:
// the sa values of a block are a 4-byte gather with a row stride of K/128 floats, and with register staging the compiler places every wait;
// DMA for the two code tiles is the next step, not taken here.
//   Bank arithmetic. A fragment read is two ds_read_b128 a lane: the 16-byte chunks c = 2 g and 2 g + 1 of row j. The LDS serves a b128 read 16
//   lanes at a time (16 x 16 = 256 bytes = the 64 banks once); unswizzled, the 16 lanes j = 0 ... 15 of one g sit at byte 128 j + 16 c: bank
//   (32 j + 4 c) % 64, only two distinct bank quads -- an 8-way conflict. The chunk is stored at c ^ ((row >> 1) & 7): even rows keep banks
//   0 ... 31, odd rows 32 ... 63, and the eight even (eight odd) rows of a 16-row sub-tile have eight distinct row >> 1 & 7, so eight distinct
//   chunks = 32 distinct banks in their half: conflict-free. The fill writes 16 consecutive lanes = the 8 chunks of rows 2 i and 2 i + 1:
//   the same argument, conflict-free.
//   Register budget before the compiler: master accumulators 64, weight fragments 4 x 8 = 32, one activation fragment 8, one MFMA result 4,
//   staging 2 x 4 x 4 + 1 = 33, addresses ~ 20: ~ 165 VGPRs, no spill expected at 512 a lane (one wave a SIMD).
// Edge tiles in M and N clamp the row index on load and mask on store. Element offsets are 64-bit.
//
// The master accumulators are fp32 VGPRs throughout. cln_mfma_keep behind every MFMA (common.h: the destination must not overlap a dying
// operand). The units are built without packed fp32 ops (_build.py), and this file writes none.
#pragma once
#include "common.h"
#include "paged_bf16.cuh"  // bf16_t, b4

namespace g8 {

typedef int i8v __attribute__((ext_vector_type(8)));
constexpr int kBlock = 128;  // the scale block in K = the K of one MFMA
constexpr int kPF = 4;       // skinny: K blocks of weights in flight a wave
constexpr int kTileM = 128, kTileN = 128, kTileThreads = 256;
constexpr int kSkinnyMaxM = 64, kCUs = 256;

struct Args {
  const uint8_t *a, *b;  // [M,K], [N,K] e4m3fn
  const float *sa, *sb;  // [M,KB], [ceil(N/128),KB]
  bf16_t* out;           // [M,N]
  int M, N, KB;          // KB = K / 128
};

// one K block on the matrix pipe: t = sum over the block's 128 k of w[n0 + 4 g + r, k] x[m0 + j, k], r = 0 ... 3
__device__ __forceinline__ f4 mfma128(const i8v& w, const i8v& x) {
  const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  // cbsz = 0, blgp = 0: both operands e4m3. Scale operands 0 with op_sel 0 select the instruction's unscaled form (scale 1.0)
  const f4 t = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, zero, 0, 0, 0, 0, 0, 0);
  cln_mfma_keep(t, w, x);
  return t;
}

__device__ __forceinline__ i8v cat(const u4& lo, const u4& hi) {
  return i8v{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}
// the 32 bytes of a lane's operand: row `row` (64-bit element offset), K block kb, K slice g
__device__ __forceinline__ i8v load_frag(const uint8_t* base, size_t row, int KB, int kb, int g) {
  const u4* p = (const u4*)(base + row * ((size_t)KB * kBlock) + (size_t)kb * kBlock + 32u * g);
  return cat(p[0], p[1]);
}
__device__ __forceinline__ void scale_add(f4& acc, const f4& t, float s) {
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = __builtin_fmaf(s, t[r], acc[r]);
}
__device__ __forceinline__ void store4(const Args& a, int m, int n, const f4& acc) {
  if (m < a.M && n < a.N) *(b4*)(a.out + (size_t)m * a.N + n) = fa2b::round4(acc);  // n % 4 == 0 and N % 8 == 0: all four or none
}

// ---- the skinny form: blockDim.x = 64 W, wave w of workgroup x owns the weight rows 16 (W x + w) ... + 15 and m = 0 ... 16 MT - 1
template <int MT>
__device__ __forceinline__ void skinny(const Args& a) {
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int n0 = 16 * (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (n0 >= a.N) return;  // a whole wave: there is no barrier in this form
  const int KB = a.KB;
  const size_t wrow = (size_t)min(n0 + j, a.N - 1);
  size_t xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = (size_t)min(16 * mt + j, a.M - 1);
  const float* sbp = a.sb + (size_t)(n0 / kBlock) * KB;  // uniform over the wave (and the workgroup)

  i8v wq[kPF];  // the weight ring: wq[i] holds K block kb with kb % kPF == i
#pragma unroll
  for (int i = 0; i < kPF; ++i) wq[i] = load_frag(a.b, wrow, KB, min(i, KB - 1), g);
  i8v xn[MT];   // the activation fragments and scales of the coming K block
  float sn[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    xn[mt] = load_frag(a.a, xrow[mt], KB, 0, g);
    sn[mt] = a.sa[xrow[mt] * KB];
  }
  f4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  for (int kb0 = 0; kb0 < KB; kb0 += kPF) {
#pragma unroll
    for (int i = 0; i < kPF; ++i) {
      const int kb = kb0 + i;
      if (kb < KB) {
        const i8v w = wq[i];
        i8v x[MT];
        float s[MT];
        const float sb = sbp[kb];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          x[mt] = xn[mt];
          s[mt] = sn[mt] * sb;
        }
        // refill: the weights kPF blocks ahead, the activations one block ahead (indices clamped: a block past the end is loaded and dropped)
        wq[i] = load_frag(a.b, wrow, KB, min(kb + kPF, KB - 1), g);
        const int k1 = min(kb + 1, KB - 1);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          xn[mt] = load_frag(a.a, xrow[mt], KB, k1, g);
          sn[mt] = a.sa[xrow[mt] * KB + k1];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) scale_add(acc[mt], mfma128(w, x[mt]), s[mt]);
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) store4(a, 16 * mt + j, n0 + 4 * g, acc[mt]);
}

// ---- the tile form
constexpr int kSlotBytes = kTileN * kBlock + kTileM * kBlock + kTileM * 4;  // codes of b, codes of a, sa
constexpr int kTileLds = 2 * kSlotBytes;
// byte offset of 16-byte chunk c of row r inside a 128 x 128 code tile
__device__ __forceinline__ unsigned swz(unsigned r, unsigned c) { return r * kBlock + ((c ^ ((r >> 1) & 7u)) << 4); }

struct Stage {  // a thread's part of one K block on its way to LDS: 4 chunks of each operand, one sa
  u4 w[4], x[4];
  float s;
};

// rows m_t ... m_t + 127 of a (the caller's: 128 blockIdx.y, or 128 t on the view of one expert), columns 128 blockIdx.x ...
__device__ __forceinline__ void tile(const Args& a, int m_t, unsigned char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int n_t = kTileN * blockIdx.x;
  const int wn = 64 * (wave & 1), wm = 64 * (wave >> 1);
  const int KB = a.KB;
  const size_t ldk = (size_t)KB * kBlock;
  // the fill: chunk c = tid & 7 of rows (tid >> 3) + 32 p, p = 0 ... 3
  const unsigned fr = tid >> 3, fc = tid & 7;
  const uint8_t *wsrc[4], *xsrc[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    wsrc[p] = a.b + (size_t)min(n_t + (int)fr + 32 * p, a.N - 1) * ldk + 16u * fc;
    xsrc[p] = a.a + (size_t)min(m_t + (int)fr + 32 * p, a.M - 1) * ldk + 16u * fc;
  }
  const float* ssrc = a.sa + (size_t)min(m_t + (tid & 127), a.M - 1) * KB;  // threads 0 ... 127 carry the sa of row tid
  const float* sbp = a.sb + (size_t)blockIdx.x * KB;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;

  auto fetch = [&](Stage& st, int kb) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      st.w[p] = *(const u4*)(wsrc[p] + (size_t)kb * kBlock);
      st.x[p] = *(const u4*)(xsrc[p] + (size_t)kb * kBlock);
    }
    st.s = ssrc[kb];
  };
  auto put = [&](const Stage& st, int slot) {
    const unsigned base = lds0 + slot * kSlotBytes;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      lds_st<u4>(base + swz(fr + 32 * p, fc), st.w[p]);
      lds_st<u4>(base + kTileN * kBlock + swz(fr + 32 * p, fc), st.x[p]);
    }
    if (tid < kTileM) lds_st<float>(base + (kTileN + kTileM) * kBlock + 4u * tid, st.s);
  };
  auto frag = [&](unsigned tile_base, unsigned row) {  // the lane's 32 bytes: chunks 2 g and 2 g + 1 of row `row`
    return cat(lds_ld<u4>(tile_base + swz(row, 2u * g)), lds_ld<u4>(tile_base + swz(row, 2u * g + 1u)));
  };

  f4 acc[4][4];  // [nt][mt]
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  Stage st;
  fetch(st, 0);
  put(st, 0);
  __syncthreads();
  for (int kb = 0; kb < KB; ++kb) {
    const unsigned base = lds0 + (kb & 1) * kSlotBytes;
    if (kb + 1 < KB) fetch(st, kb + 1);  // in flight under this block's MFMAs
    const float sb = sbp[kb];
    i8v w[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) w[nt] = frag(base, wn + 16 * nt + j);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const i8v x = frag(base + kTileN * kBlock, wm + 16 * mt + j);
      const float s = lds_ld<float>(base + (kTileN + kTileM) * kBlock + 4u * (wm + 16 * mt + j)) * sb;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) scale_add(acc[nt][mt], mfma128(w[nt], x), s);
    }
    // slot (kb + 1) & 1 was last read in iteration kb - 1, and every wave has passed that iteration's barrier
    if (kb + 1 < KB) put(st, (kb + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) store4(a, m_t + wm + 16 * mt + j, n_t + wn + 16 * nt + 4 * g, acc[nt][mt]);
}

}  // namespace g8
