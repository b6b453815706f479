// How the grouped block-scaled FP8 GEMMs (gemm_fp8_block128_grouped.cuh, gemm_fp8_block128_grouped_swiglu.cuh) find and split their work
// over expert offsets that live on the device: the rows of a [M_total, K] are sorted by expert, expert e owns the rows
// off[e] ... off[e + 1] - 1. The grid is a function of (M_total, E) and the form alone, and both forms are correct for any offsets. Defines no
// kernel; every function takes (off, M_total, E), not a kernel's argument block.
//
// OFFSETS. Read through the family's clamp (dsa_varlen_row.cuh): every value to [0, M_total], M_e = max(off[e + 1] - off[e], 0) on the
// clamped values, so every row a workgroup forms is below M_total whatever the array holds. A row in front of off[0] or at or behind off[E]
// belongs to no expert: no workgroup reads or writes it. M_e = 0 is allowed anywhere. e comes from blockIdx (skinny) or from a search whose
// every operand is workgroup-uniform (tile), the results through v_readfirstlane: the offsets arrive by scalar loads, and everything that
// depends on them -- the expert's base pointers, its row count -- stays scalar.
//
// SKINNY. Grid y = E: workgroup (x, e) owns ALL rows of expert e. It reads off[e], off[e + 1] and returns before its first weight load when
// M_e = 0: an untouched expert costs two scalar loads a workgroup and no HBM byte of weights.
//
// TILE. Row tiles of 128, in grid y
//   slots = floor(M_total / 128) + E
// of which expert e owns those from s_e = floor(off[e] / 128) + e (the scheme of flash_attn_prefill_paged_varlen.cuh).
// floor((x + y) / 128) >= floor(x / 128) + floor(y / 128) gives s_{e+1} >= s_e + ceil(M_e / 128): the ranges are disjoint, s is strictly
// increasing (also across empty experts), every tile has a slot below `slots`, at most E slots are empty. A workgroup finds the largest e with
// s_e <= its slot by binary search, ceil(log2(E + 1)) dependent scalar loads; tile t = slot - s_e of the expert is the rows off[e] + 128 t ...,
// and the workgroup returns when 128 t >= M_e.
#pragma once
#include "gemm_fp8_block128_core.cuh"  // g8::kTileM

namespace g8o {

// ---- the device side
__device__ __forceinline__ int clamped_offset(const int* off, int M, int i) { return min(max(off[i], 0), M); }

struct Rows {  // an expert's rows: c0 ... c0 + Me - 1
  int c0, Me;
};
__device__ __forceinline__ Rows expert_rows(const int* off, int M, int e) {
  const int c0 = __builtin_amdgcn_readfirstlane(clamped_offset(off, M, e));
  return {c0, __builtin_amdgcn_readfirstlane(max(clamped_offset(off, M, e + 1) - c0, 0))};
}

// first slot of expert e whose (clamped) first row is c
__device__ __forceinline__ unsigned slot_of(int c, int e) { return (unsigned)c / (unsigned)g8::kTileM + (unsigned)e; }

// The largest e in [0, E) with s_e <= slot, or -1 (a slot in front of the first expert).
__device__ __forceinline__ int expert_of_slot(const int* off, int M, int E, unsigned slot) {
  int lo = 0, hi = E;  // s_e <= slot for every e < lo, s_e > slot for every e >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (slot_of(clamped_offset(off, M, mid), mid) <= slot)
      lo = mid + 1;
    else
      hi = mid;
  }
  return __builtin_amdgcn_readfirstlane(lo - 1);
}

struct Tile {  // row tile t of expert e, whose rows are c0 ... c0 + Me - 1
  int e, c0, Me, t;
};
// The tile of a slot, or false: a slot in front of the first expert or behind the expert's last tile (M_e = 0: every one). Uniform over the
// workgroup: the caller returns on false before any barrier.
__device__ __forceinline__ bool tile_of_slot(const int* off, int M, int E, unsigned slot, Tile* w) {
  const int e = expert_of_slot(off, M, E, slot);
  if (e < 0) return false;
  const Rows r = expert_rows(off, M, e);
  const unsigned t = slot - slot_of(r.c0, e);
  if (t >= (unsigned)((r.Me + g8::kTileM - 1) / g8::kTileM)) return false;
  *w = {e, r.c0, r.Me, (int)t};
  return true;
}

// ---- the host side: the form and the grid's y, a function of (M_total, E, form) only
enum { kAuto = 0, kSkinny = 1, kTile = 2 };
constexpr long long kMaxGridY = 65535;

// The fixed rule of form = auto: skinny up to a mean group of kSkinnyMeanRows rows. The dense rule on the mean group (64) was the start;
// measured, skinny is ahead at a mean of 2 rows and below, the tile form at 8 (3 rows of 4), 16 and above; no row of the
// fused gate/up form has moved it.
constexpr int kSkinnyMeanRows = 4;
inline bool auto_skinny(long long M, long long E) { return M <= kSkinnyMeanRows * E; }

// Behind the caller's own shape check (whose -2 comes first): -2 for a launch past the grid in the form chosen; then *tile and *gy are set,
// and the status is -1 for a form that is none of 0, 1, 2.
inline int plan_form(long long M, long long E, int form, int* tile, unsigned* gy) {
  *tile = !(form == kSkinny || (form != kTile && auto_skinny(M, E)));
  const long long y = *tile ? M / g8::kTileM + E : E;
  if (y > kMaxGridY) return CLN_ERR_UNSUPPORTED;
  *gy = (unsigned)y;
  return form == kAuto || form == kSkinny || form == kTile ? CLN_OK : CLN_ERR_BAD_ARG;
}

// why the form of a describe text is what it is
inline void why_form(char* buf, size_t len, long long M, long long E, int form, int tile) {
  if (form == kAuto)
    snprintf(buf, len, "by the rule: M_total %s %d E", tile ? ">" : "<=", kSkinnyMeanRows);
  else
    snprintf(buf, len, "pinned; the rule gives %s", auto_skinny(M, E) ? "skinny" : "tile");
}

}  // namespace g8o
