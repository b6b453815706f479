// What the two MXFP4-weight GEMMs on the scaled FP4 x FP8 matrix instruction of gfx950 share: the dense form (gemm_mxfp4.cuh)
// and the grouped form over expert offsets (gemm_mxfp4_grouped.cuh) include this header and nothing of one another. It owns the constants, the
// one instruction (mfma_mx), the operand and scale loads, the weight tile's swizzle and the two bodies both forms run: skinny<MT> and tile,
// whose first row and base pointers are the caller's. It defines no kernel, no plan and no launch.
//   out[m, n] = bf16_rne( bias[n] + sum_{kb < K/32} 2^(sa[m, kb] - 127) 2^(sb[n, kb] - 127) sum_{k in block kb} e4m3(a[m, k]) e2m1(b[n, k]) )
// a [M, K] e4m3fn codes, sa [M, K/32] e8m0 bytes (what quant_mxfp8_bf16 writes); b [N, K/2] bytes of two e2m1 codes, element 2 i in the low
// nibble of byte i, sb [N, K/32] e8m0 bytes: the OCP MX formats, a gpt-oss expert's `_blocks` / `_scales` as stored. K % 32 == 0 only: the
// hidden size of gpt-oss is 2880 = 22.5 x 128.
//
// THE INSTRUCTION. v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = 4 (SrcA is e2m1, 4 VGPRs), blgp = 0 (SrcB is e4m3, 8 VGPRs) and both scale
// operands live: four MX blocks of both operands per instruction, the scales applied inside the matrix pipe, the fp32 accumulator carried
// through the C operand from one K step to the next. There is no fp32 work in either K loop: the scale_add chain of the FP8 family
// (gemm_fp8_block128_core.cuh: four v_fma_f32 per sub-tile and K block) has no counterpart here.
//
// ORIENTATION: the FP8 core's. The weight rows n are SrcA, the activation rows m SrcB. With g = lane / 16 and j = lane % 16, at K step kb:
//   SrcA, 4 VGPRs: the 16 bytes b[n0 + j, 64 kb + 16 g ... + 15] = the 32 codes k = 128 kb + 32 g ... + 31, in memory order
//   SrcB, 8 VGPRs: the 16 bytes a[m0 + j, 128 kb + 16 g ... + 15] (VGPRs 0 ... 3) and a[m0 + j, 128 kb + 64 + 16 g ... + 15] (VGPRs 4 ... 7)
//   scale A:       the byte sb[n0 + j, 4 kb + g] in bits 7:0 of the lane's scale VGPR (op_sel 0)
//   scale B:       the byte sa[m0 + j, 4 kb + g] likewise
//   D, 4 VGPRs:    D[r] = the sum for n = n0 + 4 g + r, m = m0 + j: four consecutive n of ONE m
// The matrix pipe reads the two formats differently, MEASURED with one-hot rows on both sides: an e2m1 lane holds the 32
// consecutive k of MX block g; an 8-bit lane holds two runs of 16, k = 16 g ... and k = 64 + 16 g ..., i.e. halves of the blocks g / 2 and
// 2 + g / 2. The scale byte of lane (j, g) belongs to block g of row j on BOTH sides whatever elements the lane holds. (The FP8 family loads
// both operands by one rule, so its dot product never saw the difference.) The one-hot test with a distinct scale in every (row, block) pins
// the nibble order, the lane group <-> K mapping of either side, the row <-> lane and the scale byte <-> lane mappings
// (tests/test_gpu_gemm_mxfp4.py). The scale rows have a stride of K/32 bytes (90 at K = 2880): they are read with byte loads, never as dwords.
//
// THE LAST K STEP when K % 128 != 0: an MX block at or beyond K gets a ZERO weight operand in the lane that holds it; every offset that
// would pass the row is clamped into it (weights and scales to the last MX block, an activation run of 16 to K - 16: nothing is read past a
// row). e2m1 has no NaN, the clamped activation codes and scales are real ones of the same row (finite by the caller's contract), so the
// products of such a block are exactly 0.
//
// SKINNY (decode, bound by weight bytes: N K / 2 once). A workgroup of W waves (2 or 4) owns a strip of 16 W weight rows and all of the rows
// it is given (at most 16 MT, MT in {1, 2, 4}; indices clamped on load, stores masked). The weight nibbles go from global memory straight into
// the four operand VGPRs, 16 contiguous bytes a lane and K step (16-byte aligned: K % 32 == 0), through a ring of kPF = 8 steps in registers
// with their scale bytes: 128 bytes a lane in flight, the depth of the FP8 form's ring in bytes, twice its depth in K. The activation
// fragments and their scale bytes arrive one step ahead. No LDS, no barrier, no split over K.
//   Register budget, MT = 4, before the compiler: weight ring 8 x 4 = 32, its scale bytes 8, activations 2 x 4 x 8 = 64, their scale bytes
//   2 x 4 = 8, accumulators 4 x 4 = 16, addresses ~ 20: ~ 150 VGPRs. (What hipcc reports stands in DESIGN 4.4.32.)
//
// TILE (prefill). Four waves, output tile 128 (m) x 128 (n), wave w owns n in [64 (w & 1), +64), m in [64 (w >> 1), +64): 4 x 4 sub-tiles, 64
// accumulators chained through C. Per K step an LDS slot holds 128 x 64 bytes of weight nibbles, 128 x 128 bytes of activation codes and
// 2 x 128 x 4 scale bytes = 25600 bytes; a ring of 2 slots, 51200 bytes static. The ring is filled through registers (2 + 4 16-byte global
// loads and four byte loads a thread, issued in front of the step's MFMAs, written to the other slot behind them), one barrier a step. A
// thread of the fill zeroes a weight chunk at or beyond K, so the compute loop knows nothing of the edge. LDS-DMA is the next step.
//   Bank arithmetic, weights. A row is 64 bytes = 4 chunks of 16; a fragment read is ONE ds_read_b128 a lane: chunk g of row j. The LDS serves
//   a b128 read 16 lanes at a time (256 bytes = the 64 banks once). Unswizzled, the 16 lanes j of one g sit at byte 64 j + 16 g: bank
//   (16 j + 4 g) % 64, which depends on j % 4 only -- four bank quads, a 4-way conflict. The FP8 tile's c ^ ((r >> 1) & 7) assumes 8 chunks
//   a row and does not apply. Here the chunk is stored at c ^ ((r >> 2) & 3): rows j, j + 4, j + 8, j + 12 share a 16-bank window and have
//   four distinct r >> 2 & 3, so four distinct chunks; with the four windows of j % 4 that is 16 distinct bank quads: conflict-free. The fill
//   writes 16 consecutive lanes = the 4 chunks of rows 4 i ... 4 i + 3, one r >> 2: a permutation inside each row, conflict-free.
//   The activation tile has 128-byte rows and keeps the FP8 core's swizzle (g8::swz); a fragment is its chunks g and 4 + g, and the
//   swizzle's argument holds for any chunk: eight even (odd) rows, eight distinct r >> 1 & 7, 32 distinct banks in their half. A scale byte
//   is read with ds_read_u8 at 4 row + g: 16 distinct dwords a read, the four g of a row share one (a broadcast).
//   Register budget before the compiler: accumulators 64, weight fragments 4 x 4 = 16 and their scale bytes 4, one activation fragment 8 and
//   its scale byte 1, staging 2 x 4 + 4 x 4 + 1 = 25, addresses ~ 24: ~ 145 VGPRs, no spill expected.
// Edge tiles in M and N clamp the row index on load and mask on store. Element offsets are 64-bit. cln_mfma_keep stands behind every MFMA.
#pragma once
#include "gemm_fp8_block128_core.cuh"  // g8::i8v, g8::cat, g8::swz, the tile and CU constants

namespace gx4 {

using g8::i8v;
using g8::kCUs;
using g8::kSkinnyMaxM;
using g8::kTileM;
using g8::kTileN;
constexpr int kStep = 128;  // the K of one MFMA = four MX blocks
constexpr int kMx = 32;     // the MX block
constexpr int kPF = 8;      // skinny: K steps of weights in flight a wave

struct Args {
  const uint8_t *a, *b;    // [M,K] e4m3fn, [N,K/2] two e2m1 a byte
  const uint8_t *sa, *sb;  // [M,K/32], [N,K/32] e8m0
  const bf16_t* bias;      // [N], or null
  bf16_t* out;             // [M,N]
  int M, N, K;
};

// the arguments on the rows m0 ... m0 + rows - 1 alone
__device__ __forceinline__ Args rows_view(const Args& a, int m0, int rows) {
  const size_t r = (size_t)m0;
  return {a.a + r * (size_t)a.K, a.b, a.sa + r * (size_t)(a.K / kMx), a.sb, a.bias, a.out + r * (size_t)a.N, rows, a.N, a.K};
}

// one K step: c + sum over the four MX blocks of the step, each lane's own block under its own two scale bytes (sw, sx: bits 7:0)
__device__ __forceinline__ f4 mfma_mx(const u4& w, int sw, const i8v& x, int sx, const f4& c) {
  const i8v w8 = {(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};  // an e2m1 operand is the low four of the eight
  // cbsz = 4: SrcA e2m1; blgp = 0: SrcB e4m3; op_sel 0 on both scales: byte 0 of the lane's scale VGPR
  const f4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w8, x, c, 4, 0, 0, sw, 0, sx);
  cln_mfma_keep(d, w, x);
  return d;
}

// A lane's element offset in its row at K step kb: its MX block (weights, both scales), clamped to the row's last one.
__device__ __forceinline__ int slice(int K, int kb, int g) { return min(kStep * kb + kMx * g, K - kMx); }
// The lane's two runs of 16 activation codes at K step kb, each clamped into the row.
__device__ __forceinline__ i8v load_x(const uint8_t* row, int K, int kb, int g) {
  const int k = kStep * kb + 16 * g;
  return g8::cat(*(const u4*)(row + min(k, K - 16)), *(const u4*)(row + min(k + 64, K - 16)));
}

// bias[n ... n + 3] in fp32 (n % 4 == 0; n clamped into the row for the lanes whose store is masked), or zero
__device__ __forceinline__ f4 bias4(const Args& a, int n) {
  if (!a.bias) return f4{0.0f, 0.0f, 0.0f, 0.0f};
  const b4 v = *(const b4*)(a.bias + min(n, a.N - 4));
  return f4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
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
  const int K = a.K, KS = (K + kStep - 1) / kStep;
  const size_t wrow = (size_t)min(n0 + j, a.N - 1);
  const uint8_t* wp = a.b + wrow * (size_t)(K / 2);
  const uint8_t* wsp = a.sb + wrow * (size_t)(K / kMx);
  const uint8_t *xp[MT], *xsp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const size_t xrow = (size_t)min(16 * mt + j, a.M - 1);
    xp[mt] = a.a + xrow * (size_t)K;
    xsp[mt] = a.sa + xrow * (size_t)(K / kMx);
  }

  u4 wq[kPF];  // the weight ring: wq[i], ws[i] hold K step kb with kb % kPF == i
  int ws[kPF];
#pragma unroll
  for (int i = 0; i < kPF; ++i) {
    const int k = slice(K, i, g);
    wq[i] = *(const u4*)(wp + (k >> 1));
    ws[i] = wsp[k >> 5];
  }
  i8v xn[MT];  // the activation fragments and scale bytes of the coming K step
  int sn[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    xn[mt] = load_x(xp[mt], K, 0, g);
    sn[mt] = xsp[mt][slice(K, 0, g) >> 5];
  }
  const f4 bias = bias4(a, n0 + 4 * g);
  f4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = bias;

  for (int kb0 = 0; kb0 < KS; kb0 += kPF) {
#pragma unroll
    for (int i = 0; i < kPF; ++i) {
      const int kb = kb0 + i;
      if (kb < KS) {
        const bool live = kStep * kb + kMx * g < K;  // false in the last step only, for the slices at or beyond K
        const u4 w = live ? wq[i] : u4{0u, 0u, 0u, 0u};
        const int sw = ws[i];
        i8v x[MT];
        int s[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          x[mt] = xn[mt];
          s[mt] = sn[mt];
        }
        // refill: the weights kPF steps ahead, the activations one step ahead (offsets clamped: a step past the end is loaded and dropped)
        const int kw = slice(K, kb + kPF, g), kx = slice(K, kb + 1, g);
        wq[i] = *(const u4*)(wp + (kw >> 1));
        ws[i] = wsp[kw >> 5];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          xn[mt] = load_x(xp[mt], K, kb + 1, g);
          sn[mt] = xsp[mt][kx >> 5];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma_mx(w, sw, x[mt], s[mt], acc[mt]);
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) store4(a, 16 * mt + j, n0 + 4 * g, acc[mt]);
}

// all rows of `a` in chunks of 16 MT (skinny<MT> on a view of each chunk); rows <= 16 MT is one pass
template <int MT>
__device__ __forceinline__ void skinny_rows(const Args& a) {
  for (int m0 = 0; m0 < a.M; m0 += 16 * MT) skinny<MT>(rows_view(a, m0, min(16 * MT, a.M - m0)));
}

// ---- the tile form
constexpr int kWBytes = kTileN * kStep / 2, kXBytes = kTileM * kStep, kSBytes = 4 * (kTileN + kTileM);
constexpr int kSlotBytes = kWBytes + kXBytes + kSBytes;  // nibbles of b, codes of a, scale bytes of b then of a
constexpr int kTileLds = 2 * kSlotBytes;
// byte offset of 16-byte chunk c (0 ... 3) of row r inside the 128 x 64 weight tile
__device__ __forceinline__ unsigned swz4(unsigned r, unsigned c) { return r * (kStep / 2) + ((c ^ ((r >> 2) & 3u)) << 4); }

struct Stage {  // a thread's part of one K step on its way to LDS: 2 weight chunks, 4 activation chunks, one row's four scale bytes
  u4 w[2], x[4];
  unsigned s;
};

// rows m_t ... m_t + 127 of a (the caller's: 128 blockIdx.y, or 128 t on the view of one expert), columns 128 blockIdx.x ...
__device__ __forceinline__ void tile(const Args& a, int m_t, unsigned char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int n_t = kTileN * blockIdx.x;
  const int wn = 64 * (wave & 1), wm = 64 * (wave >> 1);
  const int K = a.K, KS = (K + kStep - 1) / kStep;
  // the fill. Weights: chunk tid & 3 of rows (tid >> 2) + 64 p, p = 0, 1. Activations: chunk tid & 7 of rows (tid >> 3) + 32 p, p = 0 ... 3.
  // Scales: threads 0 ... 127 the four bytes of weight row tid, threads 128 ... 255 those of activation row tid - 128.
  const unsigned wr = tid >> 2, wc = tid & 3, xr = tid >> 3, xc = tid & 7;
  const uint8_t *wsrc[2], *xsrc[4];
#pragma unroll
  for (int p = 0; p < 2; ++p) wsrc[p] = a.b + (size_t)min(n_t + (int)wr + 64 * p, a.N - 1) * (size_t)(K / 2);
#pragma unroll
  for (int p = 0; p < 4; ++p) xsrc[p] = a.a + (size_t)min(m_t + (int)xr + 32 * p, a.M - 1) * (size_t)K;
  const uint8_t* ssrc = tid < kTileN ? a.sb + (size_t)min(n_t + tid, a.N - 1) * (size_t)(K / kMx)
                                     : a.sa + (size_t)min(m_t + tid - kTileN, a.M - 1) * (size_t)(K / kMx);
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;

  auto fetch = [&](Stage& st, int kb) {
    const int kw = kStep * kb + kMx * (int)wc;  // the weight chunk's first element: one MX block
    const u4 w0 = *(const u4*)(wsrc[0] + (min(kw, K - kMx) >> 1)), w1 = *(const u4*)(wsrc[1] + (min(kw, K - kMx) >> 1));
    st.w[0] = kw < K ? w0 : u4{0u, 0u, 0u, 0u};
    st.w[1] = kw < K ? w1 : u4{0u, 0u, 0u, 0u};
    const int kx = min(kStep * kb + 16 * (int)xc, K - 16);  // 16 activation codes a chunk
#pragma unroll
    for (int p = 0; p < 4; ++p) st.x[p] = *(const u4*)(xsrc[p] + kx);
    unsigned s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s |= (unsigned)ssrc[min(4 * kb + i, K / kMx - 1)] << (8 * i);
    st.s = s;
  };
  auto put = [&](const Stage& st, int slot) {
    const unsigned base = lds0 + slot * kSlotBytes;
#pragma unroll
    for (int p = 0; p < 2; ++p) lds_st<u4>(base + swz4(wr + 64 * p, wc), st.w[p]);
#pragma unroll
    for (int p = 0; p < 4; ++p) lds_st<u4>(base + kWBytes + g8::swz(xr + 32 * p, xc), st.x[p]);
    lds_st<unsigned>(base + kWBytes + kXBytes + 4u * tid, st.s);
  };

  f4 acc[4][4];  // [nt][mt]
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const f4 bias = bias4(a, n_t + wn + 16 * nt + 4 * g);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = bias;
  }

  Stage st;
  fetch(st, 0);
  put(st, 0);
  __syncthreads();
  for (int kb = 0; kb < KS; ++kb) {
    const unsigned base = lds0 + (kb & 1) * kSlotBytes;
    if (kb + 1 < KS) fetch(st, kb + 1);  // in flight under this step's MFMAs
    u4 w[4];
    int sw[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const unsigned row = wn + 16 * nt + j;
      w[nt] = lds_ld<u4>(base + swz4(row, g));
      sw[nt] = lds_ld<uint8_t>(base + kWBytes + kXBytes + 4u * row + g);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const unsigned row = wm + 16 * mt + j, xb = base + kWBytes;
      const i8v x = g8::cat(lds_ld<u4>(xb + g8::swz(row, g)), lds_ld<u4>(xb + g8::swz(row, 4u + g)));  // the runs at 16 g and 64 + 16 g
      const int sx = lds_ld<uint8_t>(base + kWBytes + kXBytes + 4u * (kTileN + row) + g);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt][mt] = mfma_mx(w[nt], sw[nt], x, sx, acc[nt][mt]);
    }
    // slot (kb + 1) & 1 was last read in iteration kb - 1, and every wave has passed that iteration's barrier
    if (kb + 1 < KS) put(st, (kb + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) store4(a, m_t + wm + 16 * mt + j, n_t + wn + 16 * nt + 4 * g, acc[nt][mt]);
}

}  // namespace gx4
