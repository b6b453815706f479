// Grouped (mixture-of-experts) block-scaled FP8 GEMM over expert offsets that live on the device (cln_gemm_fp8_block128_grouped_bf16,
// include/cln_amd_ext.h): the rows of a [M_total, K] are sorted by expert, expert e owns the rows off[e] ... off[e + 1] - 1 and
// its own weight b[e] [N, K] with its own scale grid b_scale[e] [ceil(N/128), K/128]; for a row m of expert e
//   out[m, n] = bf16_rne( sum_kb  a_scale[m, kb] * b_scale[e, n / 128, kb] * sum_{k in block kb} fp32(a[m, k]) * fp32(b[e, n, k]) )
// A SIBLING of gemm_fp8_block128.cuh (untouched, included): its mfma128, load_frag, scale_add, swz, Stage, store4 and its whole skinny body
// are used as they are, so the arithmetic of an element -- one v_mfma_f32_16x16x128_f8f6f4 per scale block with a zero C operand,
// s = sa * sb, fmaf in ascending kb, one rounding -- is the dense entry's, and an expert's rows carry the bits the dense entry gives on that
// expert alone, in either form. What is new here is how the work is FOUND and SPLIT when the host cannot see the offsets: the grid is a
// function of (M_total, E, N, K) alone, and both forms are correct for any offsets.
//
// OFFSETS. Read through the family's clamp (dsa_varlen_row.cuh): every value to [0, M_total], M_e = max(off[e + 1] - off[e], 0) on the
// clamped values, so every row a workgroup forms is below M_total whatever the array holds. A row in front of off[0] or at or behind off[E]
// belongs to no expert: no workgroup reads or writes it. M_e = 0 is allowed anywhere. e comes from blockIdx (skinny) or from a search whose
// every operand is workgroup-uniform (tile), the results through v_readfirstlane: the offsets arrive by scalar loads, and everything that
// depends on them -- the expert's base pointers, its row count -- stays scalar.
//
// SKINNY (decode: few rows an expert, bound by weight bytes). Grid (strips of 32 or 64 weight rows) x E: workgroup (x, e) owns strip x of
// expert e's weight and ALL of the expert's rows. It reads off[e], off[e + 1] and RETURNS BEFORE ITS FIRST WEIGHT LOAD when M_e = 0: an
// untouched expert costs two scalar loads a workgroup and no HBM byte of weights. Otherwise it walks the expert's rows in chunks of up to 64;
// per chunk the 16-row sub-tile count MT in {1, 2, 4} comes from the rows left (a workgroup-uniform branch over g8::skinny's three
// instantiations, called on a view of the expert: the chunk's rows as M, the expert's weight and scale grid as b, sb). The four-block
// register ring of weights is the dense form's; no LDS, no barrier. A second chunk re-reads the strip (32 or 64 x K bytes, from L2): the form
// is for experts of at most a few chunks, the rule below sends longer groups to the tile form.
//
// TILE (prefill: compute-bound). Tiles of 128 x 128, N tiles in x, and in y
//   slots = floor(M_total / 128) + E
// of which expert e owns those from s_e = floor(off[e] / 128) + e (the scheme of flash_attn_prefill_paged_varlen.cuh).
// floor((x + y) / 128) >= floor(x / 128) + floor(y / 128) gives s_{e+1} >= s_e + ceil(M_e / 128): the ranges are disjoint, s is strictly
// increasing (also across empty experts), every tile has a slot below `slots`, at most E slots are empty. A workgroup finds the largest e with
// s_e <= its slot by binary search, ceil(log2(E + 1)) dependent scalar loads; tile t = slot - s_e of the expert is the rows off[e] + 128 t ...,
// and the workgroup returns when 128 t >= M_e. The body is the dense tile form's on a view of the expert (M = M_e): row indices are clamped on
// load to the expert's OWN last row and stores are masked at the expert's end, not at M_total -- the next expert's rows belong to another
// workgroup with other weights. The swizzled two-slot LDS ring, the sa of the tile's rows in the slot, and sb (from the expert's own grid, one
// scalar load a K block) are the dense form's.
//
// Element offsets are 64-bit, e N K included (256 x 4096 x 7168 is 7.5e9 bytes). One launch, nothing read on the host, no workspace, no
// atomics; deterministic; graph-capturable with the offsets changing between replays. cln_mfma_keep stands behind every MFMA (inside
// g8::mfma128). The unit is built without packed fp32 ops (_build.py), and this file writes none.
#pragma once
#include "gemm_fp8_block128.cuh"

namespace g8g {

using g8::kBlock;
using g8::kSlotBytes;
using g8::kTileM;
using g8::kTileN;

struct Args {
  const uint8_t *a, *b;  // [M,K], [E,N,K] e4m3fn
  const float *sa, *sb;  // [M,KB], [E,NB,KB]
  const int* off;        // [E + 1], on the device
  bf16_t* out;           // [M,N]
  int M, E, N, KB;       // M = M_total, KB = K / 128
};

__device__ __forceinline__ int clamped_offset(const Args& g, int i) { return min(max(g.off[i], 0), g.M); }

// The dense kernel's arguments on expert e alone: its weight, its scale grid, and its rows from row c0 + m0 on, `rows` of them.
__device__ __forceinline__ g8::Args expert_view(const Args& g, int e, int c0, int m0, int rows) {
  const size_t r0 = (size_t)c0 + (size_t)m0, NB = (size_t)((g.N + kBlock - 1) / kBlock);
  const size_t ldk = (size_t)g.KB * kBlock;
  return {g.a + r0 * ldk, g.b + (size_t)e * (size_t)g.N * ldk, g.sa + r0 * g.KB, g.sb + (size_t)e * NB * g.KB, g.out + r0 * g.N, rows, g.N, g.KB};
}

// ---- the skinny form: grid (strips, E), blockDim.x = 64 W
__global__ __launch_bounds__(256) void gemm_fp8_block128_grouped_skinny_mfma(const Args g) {
  const int e = blockIdx.y;
  const int c0 = __builtin_amdgcn_readfirstlane(clamped_offset(g, e));
  const int Me = __builtin_amdgcn_readfirstlane(max(clamped_offset(g, e + 1) - c0, 0));
  if (Me == 0) return;  // the empty-expert exit: nothing of b[e] has been addressed
  for (int m0 = 0; m0 < Me; m0 += 64) {
    const int rows = min(64, Me - m0);
    const g8::Args d = expert_view(g, e, c0, m0, rows);
    if (rows <= 16) g8::skinny<1>(d);
    else if (rows <= 32) g8::skinny<2>(d);
    else g8::skinny<4>(d);
  }
}

// ---- the tile form
// first slot of expert e whose (clamped) first row is c
__device__ __forceinline__ unsigned slot_of(int c, int e) { return (unsigned)c / (unsigned)kTileM + (unsigned)e; }

// The largest e in [0, E) with s_e <= slot, or -1 (a slot in front of the first expert).
__device__ __forceinline__ int expert_of_slot(const Args& g, unsigned slot) {
  int lo = 0, hi = g.E;  // s_e <= slot for every e < lo, s_e > slot for every e >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (slot_of(clamped_offset(g, mid), mid) <= slot)
      lo = mid + 1;
    else
      hi = mid;
  }
  return __builtin_amdgcn_readfirstlane(lo - 1);
}

// g8::tile on the expert view d, with the tile's first row m_t (relative to the expert) handed in where the dense form takes it from blockIdx.y
__device__ __forceinline__ void tile(const g8::Args& d, int m_t, unsigned char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int n_t = kTileN * blockIdx.x;
  const int wn = 64 * (wave & 1), wm = 64 * (wave >> 1);
  const int KB = d.KB;
  const size_t ldk = (size_t)KB * kBlock;
  // the fill: chunk c = tid & 7 of rows (tid >> 3) + 32 p, p = 0 ... 3; activation rows clamped to the expert's own last row
  const unsigned fr = tid >> 3, fc = tid & 7;
  const uint8_t *wsrc[4], *xsrc[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    wsrc[p] = d.b + (size_t)min(n_t + (int)fr + 32 * p, d.N - 1) * ldk + 16u * fc;
    xsrc[p] = d.a + (size_t)min(m_t + (int)fr + 32 * p, d.M - 1) * ldk + 16u * fc;
  }
  const float* ssrc = d.sa + (size_t)min(m_t + (tid & 127), d.M - 1) * KB;  // threads 0 ... 127 carry the sa of row tid
  const float* sbp = d.sb + (size_t)blockIdx.x * KB;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;

  auto fetch = [&](g8::Stage& st, int kb) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      st.w[p] = *(const u4*)(wsrc[p] + (size_t)kb * kBlock);
      st.x[p] = *(const u4*)(xsrc[p] + (size_t)kb * kBlock);
    }
    st.s = ssrc[kb];
  };
  auto put = [&](const g8::Stage& st, int slot) {
    const unsigned base = lds0 + slot * kSlotBytes;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      lds_st<u4>(base + g8::swz(fr + 32 * p, fc), st.w[p]);
      lds_st<u4>(base + kTileN * kBlock + g8::swz(fr + 32 * p, fc), st.x[p]);
    }
    if (tid < kTileM) lds_st<float>(base + (kTileN + kTileM) * kBlock + 4u * tid, st.s);
  };
  auto frag = [&](unsigned tile_base, unsigned row) {  // the lane's 32 bytes: chunks 2 g and 2 g + 1 of row `row`
    return g8::cat(lds_ld<u4>(tile_base + g8::swz(row, 2u * g)), lds_ld<u4>(tile_base + g8::swz(row, 2u * g + 1u)));
  };

  f4 acc[4][4];  // [nt][mt]
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

  g8::Stage st;
  fetch(st, 0);
  put(st, 0);
  __syncthreads();
  for (int kb = 0; kb < KB; ++kb) {
    const unsigned base = lds0 + (kb & 1) * kSlotBytes;
    if (kb + 1 < KB) fetch(st, kb + 1);  // in flight under this block's MFMAs
    const float sb = sbp[kb];
    g8::i8v w[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) w[nt] = frag(base, wn + 16 * nt + j);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const g8::i8v x = frag(base + kTileN * kBlock, wm + 16 * mt + j);
      const float s = lds_ld<float>(base + (kTileN + kTileM) * kBlock + 4u * (wm + 16 * mt + j)) * sb;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) g8::scale_add(acc[nt][mt], g8::mfma128(w[nt], x), s);
    }
    // slot (kb + 1) & 1 was last read in iteration kb - 1, and every wave has passed that iteration's barrier
    if (kb + 1 < KB) put(st, (kb + 1) & 1);
    __syncthreads();
  }
  // masked at d.M = the expert's end
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) g8::store4(d, m_t + wm + 16 * mt + j, n_t + wn + 16 * nt + 4 * g, acc[nt][mt]);
}

__global__ __launch_bounds__(256) void gemm_fp8_block128_grouped_tile_mfma(const Args g) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[g8::kTileLds];
  const unsigned slot = blockIdx.y;
  const int e = expert_of_slot(g, slot);
  if (e < 0) return;  // a slot in front of the first expert
  const int c0 = __builtin_amdgcn_readfirstlane(clamped_offset(g, e));
  const int Me = __builtin_amdgcn_readfirstlane(max(clamped_offset(g, e + 1) - c0, 0));
  const unsigned t = slot - slot_of(c0, e);
  if (t >= (unsigned)((Me + kTileM - 1) / kTileM)) return;  // a slot behind the expert's last tile (M_e = 0: every one); uniform, before any barrier
  tile(expert_view(g, e, c0, 0, Me), kTileM * (int)t, smem);
}

// ---- the plan: a function of (M_total, E, N, K, form) only (the entry and its describe share it)
enum { kAuto = 0, kSkinny = 1, kTile = 2 };
struct Plan {
  int tile;   // 1: the tile form
  int waves;  // waves a workgroup (skinny: 2 or 4 = a strip of 32 or 64 weight rows)
  unsigned gx, gy;
};
constexpr long long kMaxGridY = 65535;

// The fixed rule of form = auto: skinny up to a mean group of kSkinnyMeanRows rows. The dense rule on the mean group (64) was the start;
// measured, skinny is ahead at a mean of 2 rows and below, the tile form at 8 (3 rows of 4), 16 and above.
constexpr int kSkinnyMeanRows = 4;
inline bool auto_skinny(long long M, long long E) { return M <= kSkinnyMeanRows * E; }

// -2 for a shape outside the contract or past one launch in the form chosen; then -1 for a form that is none of 0, 1, 2
inline int plan(long long M, long long E, long long N, long long K, int form, Plan* p) {
  if (M < 1 || E < 1 || N < 8 || N % 8 || K < kBlock || K % kBlock) return CLN_ERR_UNSUPPORTED;
  if (M > 0x7fffffffLL || E > 0x7fffffffLL - 1 || N > 0x7fffffffLL - 256 || K > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  const bool known = form == kAuto || form == kSkinny || form == kTile;
  if (form == kSkinny || (form != kTile && auto_skinny(M, E))) {
    if (E > kMaxGridY) return CLN_ERR_UNSUPPORTED;
    p->tile = 0;
    // 64-row strips only where strips x E workgroups still give every CU one (the host cannot know how many experts are empty)
    p->waves = (N + 63) / 64 * E >= g8::kCUs ? 4 : 2;
    p->gx = (unsigned)((N + 16 * p->waves - 1) / (16 * p->waves));
    p->gy = (unsigned)E;
  } else {
    const long long slots = M / kTileM + E;
    if (slots > kMaxGridY) return CLN_ERR_UNSUPPORTED;
    p->tile = 1;
    p->waves = 4;
    p->gx = (unsigned)((N + kTileN - 1) / kTileN);
    p->gy = (unsigned)slots;
  }
  return known ? CLN_OK : CLN_ERR_BAD_ARG;
}

inline int launch(const Args& g, const Plan& p, hipStream_t stream) {
  const dim3 grid(p.gx, p.gy), block(64 * p.waves);
  if (p.tile) CLN_LAUNCH(gemm_fp8_block128_grouped_tile_mfma, grid, block, 0, stream, g);
  else CLN_LAUNCH(gemm_fp8_block128_grouped_skinny_mfma, grid, block, 0, stream, g);
  return cln_check_launch();
}

}  // namespace g8g
