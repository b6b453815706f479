// The gate/up projection of a mixture-of-experts FFN with SiLU-mul and the FP8 activation quantiser fused behind it
// (cln_gemm_fp8_block128_grouped_swiglu_fp8, include/cln_amd_ext.h): a, a_scale, expert_offsets as in
// gemm_fp8_block128_grouped.cuh; b e4m3fn [E, 2 I, K] with an expert's rows 0 ... I - 1 the gate and I ... 2 I - 1 the up projection, b_scale fp32
// [E, 2 I / 128, K / 128]; for a row m of expert e and a column c < I
//   G  = sum_kb a_scale[m, kb] * b_scale[e, c / 128, kb]           * sum_{k in kb} fp32(a[m, k]) * fp32(b[e, c, k])
//   U  = sum_kb a_scale[m, kb] * b_scale[e, I / 128 + c / 128, kb] * sum_{k in kb} fp32(a[m, k]) * fp32(b[e, I + c, k])
//   hf = (G * rcp(1 + exp(-G))) * U                                                                      (fp32; nothing is rounded to bf16)
// and per row and 128 columns of hf the rule of quant_fp8_block128_bf16.cuh (the scale: fp8_block_scale.cuh): h e4m3fn [M_total, I], h_scale
// fp32 [M_total, I / 128] -- the a, a_scale of the down projection. This header owns the two fused kernels with both of their bodies, the
// SiLU / amax / quantise epilogues, the plan and the launch. G and U are the grouped kernel's sums: one g8::mfma128 per scale block with a
// zero C operand, s = sa * sb, fmaf in ascending kb (gemm_fp8_block128_core.cuh); the clamp, the slots, the search and the form rule are
// gemm_fp8_block128_offsets.cuh's (g8o). A workgroup owns the SAME 128 columns of gate and up, so it holds every value a (row, block) scale
// needs: no workspace, no atomics, no second pass.
//   Kept here on purpose: the skinny K loop with two weight rows a lane and the two-slot LDS ring with 256 weight rows a slot. Written once in
//   the core as templates over the rows (a loop over NW in {1, 2}, a ring over WR in {128, 256}) both passed the register gate without a spill
//   and gave the same bytes, but hipcc scheduled them differently and the MI355X measured them slower than these bodies by more than the
//   0.1 - 0.3 % run-to-run spread: this skinny form 3 - 5 % at 16 and more chunks an expert, this tile form 7 - 9 % at E = 256, I = 2048,
//   K = 7168, the dense skinny form 7 - 10 % at M = 64 (profiles/r42_gemm_fp8_block128_core.log).
//
// SILU. v_exp_f32 and v_rcp_f32 (approximate, about 1 ulp each). For G >= 32, exp(-G) < 2^-46, 1 + exp(-G) rounds to 1, v_rcp_f32(1) is 1
// and G * 1 is G: the factor returns G itself, which the exact test stands on. For G < -88 the exponential is +inf, its reciprocal 0.
//
// TILE (prefill). Grid (I / 128, floor(M_total / 128) + E): column tiles x the grouped tile form's slots. A workgroup of 4 waves owns 128 rows
// x 128 columns of h and streams, per K block, a 256-row weight tile (rows 0 ... 127 gate, 128 ... 255 up), the 128 activation rows and their
// sa through the two-slot ring swizzled by g8::swz; a slot is 256 x 128 + 128 x 128 + 512 = 49664 bytes, two are 99328 (dynamic LDS: above
// 64 KiB, inside gfx950's 160 KiB). Wave w keeps the quarter rows 64 (w >> 1) ..., columns 64 (w & 1) ... of BOTH G and U: 128 fp32
// accumulators. Per K block it holds its 4 activation fragments and walks its 8 weight fragments: 12 fragment reads for 32 MFMAs (the plain
// tile: 8 for 16). Two sb values a K block, both scalar loads. Epilogue: hf in the registers of G; a row's amax over the lane's 16 values,
// over the four lane groups g by two permlane swaps, over the two waves that share the rows through 1 KiB of the (by then free) ring and one
// barrier; then one 4-byte code store a lane and sub-tile (four consecutive columns) and one float a row from one lane.
//
// SKINNY (decode). Grid (I / 128, E), 8 waves: workgroup (t, e) owns column block t of h for ALL rows of expert e, wave w the gate rows
// 128 t + 16 w ... + 15 and the up rows I + the same. Two four-block register rings of weights (gate, up): every weight byte is read by
// exactly one wave and never passes through LDS. M_e = 0 returns before the first weight load. Rows go in chunks of up to kChunk = 64, MT = 1, 2
// or 4 sub-tiles by the rows left (workgroup-uniform, as is every trip count). Per chunk each wave's 16-column partial amaxes go through
// 8 x 16 MT floats of LDS (two buffers by the chunk's parity: one barrier a chunk), then each wave converts and stores its own 16 columns.
//
// Rows are clamped on load to the expert's own last row and masked on store at the expert's end. Element offsets are 64-bit. One launch,
// nothing read on the host, deterministic, graph-capturable with the offsets changing between replays. cln_mfma_keep stands behind every MFMA
// (inside g8::mfma128). The unit is built without packed fp32 ops (_build.py), and this file writes none.
#pragma once
#include "fp8_block_scale.cuh"
#include "gemm_fp8_block128_core.cuh"
#include "gemm_fp8_block128_offsets.cuh"

namespace g8s {

using g8::kBlock;
using g8::kTileM;
using g8::kTileN;

struct Args {
  const uint8_t *a, *b;  // [M,K], [E,2I,K] e4m3fn
  const float *sa, *sb;  // [M,KB], [E,2I/128,KB]
  const int* off;        // [E + 1], on the device
  uint8_t* h;            // [M,I] e4m3fn
  float* hs;             // [M,I/128]
  int M, E, I, KB;       // M = M_total, KB = K / 128
  int pow2;
};

__device__ __forceinline__ float silu_mul(float G, float U) {
  return (G * __builtin_amdgcn_rcpf(1.0f + __expf(-G))) * U;
}

// four consecutive codes, byte r = column r: the clamp and the conversion of kva::store_fp8
__device__ __forceinline__ unsigned pack4(const f4& y, float inv) {
  float z[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) z[r] = fminf(fmaxf(y[r] * inv, -448.0f), 448.0f);
  int v = 0;
  v = __builtin_amdgcn_cvt_pk_fp8_f32(z[0], z[1], v, false);
  v = __builtin_amdgcn_cvt_pk_fp8_f32(z[2], z[3], v, true);
  return (unsigned)v;
}

// max over the four lanes j, j + 16, j + 32, j + 48 (the lane groups g of one row j), left in all four
__device__ __forceinline__ float max_over_g(float v) {
  const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(s16[0]), __uint_as_float(s16[1]));
  const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(s32[0]), __uint_as_float(s32[1]));
}

__device__ __forceinline__ float amax4(const f4& y) { return fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3]))); }

// ---- the skinny form: grid (I / 128, E), 8 waves
constexpr int kSkinnyWaves = 8, kSkinnyThreads = 64 * kSkinnyWaves;
constexpr int kChunk = 64;  // rows a chunk: MT = 4 fits the 256 registers of 512 threads without a spill (hipcc: 249)
constexpr int kSkinnyLds = 2 * kSkinnyWaves * kChunk * 4;

// One chunk: `rows` (1 ... 16 MT) rows from row r0 (absolute) of expert e. red: this chunk's [8][16 MT] floats of LDS.
template <int MT>
__device__ __forceinline__ void skinny(const Args& g, int e, size_t r0, int rows, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, gq = lane >> 4;
  const int t = blockIdx.x, KB = g.KB, NB = 2 * (g.I / kBlock);
  const uint8_t* be = g.b + (size_t)e * (size_t)(2 * (size_t)g.I) * ((size_t)KB * kBlock);
  const size_t grow = (size_t)(kTileN * t + 16 * wave + j), urow = grow + (size_t)g.I;
  size_t xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = r0 + (size_t)min(16 * mt + j, rows - 1);
  const float* sbg = g.sb + ((size_t)e * NB + (size_t)t) * KB;  // uniform over the workgroup
  const float* sbu = sbg + (size_t)(g.I / kBlock) * KB;

  g8::i8v wg[g8::kPF], wu[g8::kPF];  // the weight rings: slot i holds K block kb with kb % kPF == i
#pragma unroll
  for (int i = 0; i < g8::kPF; ++i) {
    wg[i] = g8::load_frag(be, grow, KB, min(i, KB - 1), gq);
    wu[i] = g8::load_frag(be, urow, KB, min(i, KB - 1), gq);
  }
  g8::i8v xn[MT];  // the activation fragments and scales of the coming K block
  float sn[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    xn[mt] = g8::load_frag(g.a, xrow[mt], KB, 0, gq);
    sn[mt] = g.sa[xrow[mt] * KB];
  }
  f4 accg[MT], accu[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) accg[mt] = accu[mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  for (int kb0 = 0; kb0 < KB; kb0 += g8::kPF) {
#pragma unroll
    for (int i = 0; i < g8::kPF; ++i) {
      const int kb = kb0 + i;
      if (kb < KB) {
        const g8::i8v w0 = wg[i], w1 = wu[i];
        g8::i8v x[MT];
        float s0[MT], s1[MT];
        const float sb0 = sbg[kb], sb1 = sbu[kb];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          x[mt] = xn[mt];
          s0[mt] = sn[mt] * sb0;
          s1[mt] = sn[mt] * sb1;
        }
        // refill: the weights kPF blocks ahead, the activations one block ahead (indices clamped: a block past the end is loaded and dropped)
        wg[i] = g8::load_frag(be, grow, KB, min(kb + g8::kPF, KB - 1), gq);
        wu[i] = g8::load_frag(be, urow, KB, min(kb + g8::kPF, KB - 1), gq);
        const int k1 = min(kb + 1, KB - 1);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          xn[mt] = g8::load_frag(g.a, xrow[mt], KB, k1, gq);
          sn[mt] = g.sa[xrow[mt] * KB + k1];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          g8::scale_add(accg[mt], g8::mfma128(w0, x[mt]), s0[mt]);
          g8::scale_add(accu[mt], g8::mfma128(w1, x[mt]), s1[mt]);
        }
      }
    }
  }
  // hf in the registers of G; the wave's partial amax of row 16 mt + j (its 16 columns) to LDS
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) accg[mt][r] = silu_mul(accg[mt][r], accu[mt][r]);
    const float m = max_over_g(amax4(accg[mt]));
    if (gq == 0) red[wave * (16 * MT) + 16 * mt + j] = m;
  }
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    float m = 0.0f;
#pragma unroll
    for (int w = 0; w < kSkinnyWaves; ++w) m = fmaxf(m, red[w * (16 * MT) + 16 * mt + j]);
    const float scale = cln_fp8_block_scale(m, g.pow2);
    const float inv = 1.0f / scale;
    const unsigned code = pack4(accg[mt], inv);
    if (16 * mt + j < rows) {
      const size_t row = r0 + (size_t)(16 * mt + j);
      *(unsigned*)(g.h + row * (size_t)g.I + (size_t)(kTileN * t + 16 * wave + 4 * gq)) = code;
      if (wave == 0 && gq == 0) g.hs[row * (size_t)(g.I / kBlock) + (size_t)t] = scale;
    }
  }
}

__global__ __launch_bounds__(kSkinnyThreads) void gemm_fp8_block128_grouped_swiglu_skinny_mfma(const Args g) {
  __shared__ float red[2][kSkinnyWaves * kChunk];
  const int e = blockIdx.y;
  const g8o::Rows r = g8o::expert_rows(g.off, g.M, e);
  if (r.Me == 0) return;  // the empty-expert exit: nothing of b[e] has been addressed
  int parity = 0;
  for (int m0 = 0; m0 < r.Me; m0 += kChunk, parity ^= 1) {
    const int rows = min(kChunk, r.Me - m0);
    const size_t r0 = (size_t)r.c0 + (size_t)m0;
    // a wave writes red[parity] again only behind the next chunk's barrier, which every wave reaches after its reads of this chunk
    if (rows <= 16) skinny<1>(g, e, r0, rows, red[parity]);
    else if (rows <= 32) skinny<2>(g, e, r0, rows, red[parity]);
    else skinny<4>(g, e, r0, rows, red[parity]);
  }
}

// ---- the tile form
constexpr int kWRows = 2 * kTileN;                                           // weight rows a slot: gate, then up
constexpr int kSlotBytes = kWRows * kBlock + kTileM * kBlock + kTileM * 4;  // codes of b (gate | up), codes of a, sa
constexpr int kTileLds = 2 * kSlotBytes;

struct Stage {  // a thread's part of one K block on its way to LDS: 8 chunks of the weights, 4 of the activations, one sa
  u4 w[8], x[4];
  float s;
};

// The tile of rows m_t ... of expert e (first row c0, Me rows), columns 128 blockIdx.x ...
__device__ __forceinline__ void tile(const Args& g, int e, int c0, int Me, int m_t, unsigned char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, gq = lane >> 4;
  const int t = blockIdx.x, n_t = kTileN * t;
  const int wn = 64 * (wave & 1), wm = 64 * (wave >> 1);
  const int KB = g.KB, NB = 2 * (g.I / kBlock);
  const size_t ldk = (size_t)KB * kBlock;
  const uint8_t* be = g.b + (size_t)e * (size_t)(2 * (size_t)g.I) * ldk;
  const uint8_t* ae = g.a + (size_t)c0 * ldk;
  // the fill: chunk c = tid & 7 of rows (tid >> 3) + 32 p; weight tile rows 0 ... 127 are gate rows n_t ..., 128 ... 255 up rows I + n_t ...;
  // activation rows clamped to the expert's own last row
  const unsigned fr = tid >> 3, fc = tid & 7;
  const uint8_t* wsrc = be + (size_t)(n_t + (int)fr) * ldk + 16u * fc;
  const size_t up = (size_t)g.I * ldk;
  const uint8_t* xsrc[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) xsrc[p] = ae + (size_t)min(m_t + (int)fr + 32 * p, Me - 1) * ldk + 16u * fc;
  const float* ssrc = g.sa + ((size_t)c0 + (size_t)min(m_t + (tid & 127), Me - 1)) * KB;  // threads 0 ... 127 carry the sa of row tid
  const float* sbg = g.sb + ((size_t)e * NB + (size_t)t) * KB;
  const float* sbu = sbg + (size_t)(g.I / kBlock) * KB;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  constexpr unsigned kX = kWRows * kBlock, kS = kX + kTileM * kBlock;  // the activation tile and the sa inside a slot

  auto fetch = [&](Stage& st, int kb) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      st.w[p] = *(const u4*)(wsrc + (size_t)(32 * p) * ldk + (size_t)kb * kBlock);
      st.w[4 + p] = *(const u4*)(wsrc + up + (size_t)(32 * p) * ldk + (size_t)kb * kBlock);
      st.x[p] = *(const u4*)(xsrc[p] + (size_t)kb * kBlock);
    }
    st.s = ssrc[kb];
  };
  auto put = [&](const Stage& st, int slot) {
    const unsigned base = lds0 + slot * kSlotBytes;
#pragma unroll
    for (int p = 0; p < 8; ++p) lds_st<u4>(base + g8::swz(fr + 32 * p, fc), st.w[p]);
#pragma unroll
    for (int p = 0; p < 4; ++p) lds_st<u4>(base + kX + g8::swz(fr + 32 * p, fc), st.x[p]);
    if (tid < kTileM) lds_st<float>(base + kS + 4u * tid, st.s);
  };
  auto frag = [&](unsigned tile_base, unsigned row) {  // the lane's 32 bytes: chunks 2 g and 2 g + 1 of row `row`
    return g8::cat(lds_ld<u4>(tile_base + g8::swz(row, 2u * gq)), lds_ld<u4>(tile_base + g8::swz(row, 2u * gq + 1u)));
  };

  f4 acc[8][4];  // [nt][mt]: nt 0 ... 3 gate, 4 ... 7 up (the same columns)
#pragma unroll
  for (int nt = 0; nt < 8; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  Stage st;
  fetch(st, 0);
  put(st, 0);
  __syncthreads();
  for (int kb = 0; kb < KB; ++kb) {
    const unsigned base = lds0 + (kb & 1) * kSlotBytes;
    if (kb + 1 < KB) fetch(st, kb + 1);  // in flight under this block's MFMAs
    const float sb0 = sbg[kb], sb1 = sbu[kb];
    g8::i8v x[4];
    float s0[4], s1[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      x[mt] = frag(base + kX, wm + 16 * mt + j);
      const float s = lds_ld<float>(base + kS + 4u * (wm + 16 * mt + j));
      s0[mt] = s * sb0;
      s1[mt] = s * sb1;
    }
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      const g8::i8v w = frag(base, (nt < 4 ? 0 : kTileN) + wn + 16 * (nt & 3) + j);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) g8::scale_add(acc[nt][mt], g8::mfma128(w, x[mt]), nt < 4 ? s0[mt] : s1[mt]);
    }
    // slot (kb + 1) & 1 was last read in iteration kb - 1, and every wave has passed that iteration's barrier
    if (kb + 1 < KB) put(st, (kb + 1) & 1);
    __syncthreads();
  }
  // Behind the last barrier no wave reads the ring again: its first 1 KiB is red[2][128], the two column halves' amax of every row.
  float m[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    m[mt] = 0.0f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[nt][mt][r] = silu_mul(acc[nt][mt][r], acc[4 + nt][mt][r]);
      m[mt] = fmaxf(m[mt], amax4(acc[nt][mt]));
    }
    m[mt] = max_over_g(m[mt]);
    if (gq == 0) lds_st<float>(lds0 + 4u * (kTileM * (wave & 1) + wm + 16 * mt + j), m[mt]);
  }
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int mr = m_t + wm + 16 * mt + j;  // relative to the expert; masked at the expert's end
    const float other = lds_ld<float>(lds0 + 4u * (kTileM * ((wave & 1) ^ 1) + wm + 16 * mt + j));
    const float scale = cln_fp8_block_scale(fmaxf(m[mt], other), g.pow2);
    const float inv = 1.0f / scale;
    const size_t row = (size_t)c0 + (size_t)mr;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const unsigned code = pack4(acc[nt][mt], inv);
      if (mr < Me) *(unsigned*)(g.h + row * (size_t)g.I + (size_t)(n_t + wn + 16 * nt + 4 * gq)) = code;
    }
    if (mr < Me && (wave & 1) == 0 && gq == 0) g.hs[row * (size_t)(g.I / kBlock) + (size_t)t] = scale;
  }
}

__global__ __launch_bounds__(256) void gemm_fp8_block128_grouped_swiglu_tile_mfma(const Args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  g8o::Tile w;
  if (!g8o::tile_of_slot(g.off, g.M, g.E, blockIdx.y, &w)) return;  // uniform, before any barrier
  tile(g, w.e, w.c0, w.Me, kTileM * w.t, smem);
}

// ---- the plan: a function of (M_total, E, I, K, form) only (the entry and its describe share it)
struct Plan {
  int tile;  // 1: the tile form
  unsigned gx, gy;
};

// -2 for a shape outside the contract or past one launch in the form chosen; then -1 for a form that is none of 0, 1, 2
inline int plan(long long M, long long E, long long I, long long K, int form, Plan* p) {
  if (M < 1 || E < 1 || I < kBlock || I % kBlock || K < kBlock || K % kBlock) return CLN_ERR_UNSUPPORTED;
  if (M > 0x7fffffffLL || E > 0x7fffffffLL - 1 || 2 * I > 0x7fffffffLL - 256 || K > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  p->gx = (unsigned)(I / kBlock);
  return g8o::plan_form(M, E, form, &p->tile, &p->gy);
}

inline int launch(const Args& g, const Plan& p, hipStream_t stream) {
  const dim3 grid(p.gx, p.gy);
  if (p.tile) {
    static cln_lds_attr attr;
    if (cln_ensure_lds(attr, (const void*)gemm_fp8_block128_grouped_swiglu_tile_mfma, kTileLds) != CLN_OK) return CLN_ERR_LAUNCH;
    CLN_LAUNCH(gemm_fp8_block128_grouped_swiglu_tile_mfma, grid, dim3(256), kTileLds, stream, g);
  } else {
    CLN_LAUNCH(gemm_fp8_block128_grouped_swiglu_skinny_mfma, grid, dim3(kSkinnyThreads), 0, stream, g);
  }
  return cln_check_launch();
}

}  // namespace g8s
