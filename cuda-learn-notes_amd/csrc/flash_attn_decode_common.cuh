// What the three decode attention entries share (cln_fa2_decode, cln_fa2_decode_paged, cln_fa2_decode_paged_multi: flash_attn_decode.cuh,
// flash_attn_decode_paged.cuh, flash_attn_decode_paged_multi.cuh): the softmax-partial helpers, the split of the keys of a
// (sequence, KV head) over S workgroups, the paged row address, the end of a workgroup, the kernel that merges the splits, and on the host the
// split plan and the argument checks of the C entries.
//
// Every entry gives each workgroup of 4 waves the keys [s C, min((s + 1) C, len_b)) of one (sequence, KV head). With one split the workgroup writes
// fp16 O (and the natural-log LSE); with S > 1 it writes its unnormalised fp32 O and (m, l) to the caller's workspace and fa2_decode_combine_kernel
// merges the splits of an output row in ascending s. A split that lies wholly past len_b writes nothing and the combine kernel skips it by the same
// arithmetic on len_b: no workspace cell is read that this call did not write. No atomics.
//
// Workspace layout (floats): O partials [rows][S][D], then (m, l) pairs [rows][S][2]  ->  rows S (D + 2) 4 bytes; rows = the fp16 rows of o.
#pragma once
#include "common.h"
#include <math.h>
#include <stdio.h>

namespace fa2d {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * CLN_WAVE;

#define FA2D_NEG_INF (-__builtin_huge_valf())

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// sum over the LPR (8 or 16) neighbouring lanes that share a cache row; every lane of the group gets it
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
  v += cln_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += cln_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += cln_dpp<0x141>(v);  // row_half_mirror
  if constexpr (LPR == 16) v += cln_dpp<0x140>(v);  // row_mirror
  return v;
}

// (m, l, o) <- the softmax partial of the union of two key sets; (-inf, 0, 0) is neutral
__device__ __forceinline__ void merge(float& m, float& l, float (&o)[8], float pm, float pl, const float (&po)[8]) {
  const float mx = fmaxf(m, pm);
  const float ms = mx == FA2D_NEG_INF ? 0.0f : mx;
  const float sa = ex2(m - ms), sb = ex2(pm - ms);
  l = l * sa + pl * sb;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = o[j] * sa + po[j] * sb;
  m = mx;
}

template <int WHICH>  // 16: rows 0|1 and 2|3 of the wave; 32: its two halves
__device__ __forceinline__ void swap_pair(float x, float& a, float& b) {
  if constexpr (WHICH == 16) {
    const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    a = __uint_as_float(s[0]), b = __uint_as_float(s[1]);
  } else {
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    a = __uint_as_float(s[0]), b = __uint_as_float(s[1]);
  }
}
// both partners of a permlane swap step end up with merge(first, second) of the pair, bit for bit
template <int WHICH>
__device__ __forceinline__ void merge_swap(float& m, float& l, float (&o)[8]) {
  float ma, mb, la, lb, oa[8], ob[8];
  swap_pair<WHICH>(m, ma, mb);
  swap_pair<WHICH>(l, la, lb);
#pragma unroll
  for (int j = 0; j < 8; ++j) swap_pair<WHICH>(o[j], oa[j], ob[j]);
  merge(ma, la, oa, mb, lb, ob);
  m = ma, l = la;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = oa[j];
}

// The job of workgroup blockIdx.x = (b heads + h) S + s: split s of KV head h of sequence b, logical rows lo .. lo + n - 1 of its len keys.
struct Split {
  unsigned bh, b, h, s;
  int len, lo;
  unsigned n;
};
// false: the split lies wholly past the length, the workgroup returns (the combine kernel skips it by the same arithmetic)
__device__ __forceinline__ bool split_of(Split& w, const int* __restrict__ seqlens, int heads, int Nmax, int S, int C) {
  w.bh = blockIdx.x / (unsigned)S, w.s = blockIdx.x - w.bh * (unsigned)S;
  w.b = w.bh / (unsigned)heads, w.h = w.bh - w.b * (unsigned)heads;
  w.len = min(max(seqlens[w.b], 0), Nmax);
  w.lo = (int)w.s * C;  // (S - 1) C < Nmax: no overflow
  w.n = w.len > w.lo ? (unsigned)min(C, w.len - w.lo) : 0u;
  return S == 1 || w.lo < w.len;
}

// A paged cache: pools fp16 [P,Hkv,page,D], block table int32 [B,max_pages], page = 1 << page_shift. Row r of a split resolves through the table
// entry of logical row lo + r; the entry is fetched one step before the row, so the dependent chain table -> row is off the critical path.
// At = a lane's view of its workgroup's split: its part of row r is at k / v + elem(...); `off` is the lane's own offset (in halves) inside a row.
struct PagedKV {
  const half_t *k, *v;
  const int* table;
  int Hkv, max_pages, page_shift;
  __host__ __device__ int heads() const { return Hkv; }
  __host__ __device__ int nmax() const { return max_pages << page_shift; }  // the plan checked that it fits
  struct At {
    const half_t *k, *v;
    const int* bt;
    unsigned kvh, lo;
    int off;
  };
  __device__ At at(const Split& w, int, int off) const { return {k, v, table + (size_t)w.b * max_pages, w.h, (unsigned)w.lo, off}; }
  // the physical page of row r; rows at or past n have no table entry that is ours to read
  __device__ int lookup(const At& a, unsigned r, unsigned n) const { return r < n ? a.bt[(a.lo + r) >> page_shift] : 0; }
  __device__ size_t elem(const At& a, int pg, unsigned r, int D) const {
    return ((((size_t)pg * Hkv + a.kvh) << page_shift) + ((a.lo + r) & ((1u << page_shift) - 1u))) * D + a.off;
  }
};

// Where a workgroup's results go: o fp16 [rows][D], lse fp32 [rows] or null, and for S > 1 the workspace (layout above).
struct Out {
  half_t* o;
  float *lse, *ws_o, *ws_ml;
};
inline Out make_out(void* o, float* lse, void* workspace, long long rows, int S, int D) {
  float* ws = (float*)workspace;
  return {(half_t*)o, lse, ws, S > 1 ? ws + (size_t)rows * S * D : nullptr};
}

// (mx, L, O) of one output column from the four waves' partials in LDS, waves 0 .. 3 in ascending order: (m, l) of wave i at ml[i ml_stride],
// its O column at po[i o_stride]
__device__ __forceinline__ void reduce_waves(const float* ml, int ml_stride, const float* po, int o_stride, float& mx, float& L, float& O) {
  mx = ml[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) mx = fmaxf(mx, ml[i * ml_stride]);
  const float ms = mx == FA2D_NEG_INF ? 0.0f : mx;
  L = 0.0f, O = 0.0f;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const float f = ex2(ml[i * ml_stride] - ms);
    L = fmaf(ml[i * ml_stride + 1], f, L);  // spelled out: a contraction left to the compiler may differ between two instantiations
    O = fmaf(po[i * o_stride], f, O);
  }
}

// Column t of output row `row` from its merged (mx, L, O). No visible key (L = 0): O = 0, LSE = -inf.
template <int D>
__device__ __forceinline__ void store_final(const Out& out, size_t row, int t, float mx, float L, float O) {
  const float inv = L > 0.0f ? 1.0f / L : 0.0f;
  out.o[row * D + t] = (half_t)(O * inv);
  if (out.lse && t == 0) out.lse[row] = L > 0.0f ? (mx + __builtin_log2f(L)) * 0.6931471805599453f : FA2D_NEG_INF;
}
// ... the end of a workgroup: with one split the final values, else the unnormalised partial of split s
template <int D>
__device__ __forceinline__ void store_split(const Out& out, size_t row, int t, unsigned s, int S, float mx, float L, float O) {
  if (S == 1) {
    store_final<D>(out, row, t, mx, L, O);
  } else {
    const size_t cell = row * S + s;
    out.ws_o[cell * D + t] = O;
    if (t == 0) out.ws_ml[cell * 2] = mx, out.ws_ml[cell * 2 + 1] = L;
  }
}

// One workgroup of D threads per output row: the live splits ceil(len_b / C) of its sequence, merged in ascending s. A live split may hold no key
// the row sees (its partial is (-inf, 0, 0)), and a row may see none at all: the maximum may be -inf.
template <int D>
__global__ __launch_bounds__(D) void fa2_decode_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                               const int* __restrict__ seqlens, half_t* __restrict__ o, float* __restrict__ lse,
                                                               int rows_per_seq, int Nmax, int S, int C) {
  const unsigned row = blockIdx.x;
  const int t = threadIdx.x;
  const unsigned len = (unsigned)min(max(seqlens[row / (unsigned)rows_per_seq], 0), Nmax);
  const int live = (int)((len + (unsigned)C - 1u) / (unsigned)C);  // <= S, as S C >= Nmax
  const float* ml = ws_ml + (size_t)row * S * 2;
  const float* po = ws_o + (size_t)row * S * D + t;
  float mx = FA2D_NEG_INF;
  for (int s = 0; s < live; ++s) mx = fmaxf(mx, ml[2 * s]);
  const float ms = mx == FA2D_NEG_INF ? 0.0f : mx;  // never exp2(-inf + inf)
  float L = 0.0f, O = 0.0f;
  for (int s = 0; s < live; ++s) {
    const float f = ex2(ml[2 * s] - ms);
    L = fmaf(ml[2 * s + 1], f, L);
    O = fmaf(po[(size_t)s * D], f, O);
  }
  store_final<D>(Out{o, lse, nullptr, nullptr}, row, t, mx, L, O);
}

// the status of the stream kernel's launch, then for S > 1 the combine kernel over `rows` output rows
template <int D>
int launch_combine(int rc, const Out& out, const int* seqlens, long long rows, int rows_per_seq, int Nmax, int S, int C, hipStream_t stream) {
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_combine_kernel<D>), dim3((unsigned)rows), dim3(D), 0, stream, (const float*)out.ws_o, (const float*)out.ws_ml, seqlens,
             out.o, out.lse, rows_per_seq, Nmax, S, C);
  return cln_check_launch();
}

inline float scale_log2(int D) { return (float)(1.4426950408889634 / sqrt((double)D)); }

// ---------------------------------------------------------------- host side: the plan and the checks of the C entries

inline long long workspace_bytes(long long rows, int S, int D) { return S > 1 ? rows * S * (D + 2) * 4 : 0; }

// `workgroups` of 256 threads, then `rows` workgroups of D threads, both in x; HIP takes at most 2^32 - 1 threads per grid dimension
inline bool grid_fits(long long workgroups, long long rows, int D) { return workgroups <= 0xffffffffLL / kThreads && rows <= 0xffffffffLL / D; }

struct Plan {
  int splits, chunk;
  long long ws_bytes;
};

// The split plan: a function of the shape only -- never of the lengths or the table, which stay on the device -- so the bits of a sequence do not
// depend on its neighbours. bk = the (sequence, KV head) pairs, each served by S workgroups; rows = the output rows; unit = what a chunk is a
// multiple of (the key step, or the page where that is longer). The constants come from the sweep of tools/fa_decode_probe.py:
constexpr int kTargetWorkgroups = 1024;  // split until bk S reaches four workgroups per CU ...
constexpr int kMinChunk = 256;           // ... but give no workgroup fewer keys than this ...
constexpr int kMaxSplits = 64;           // ... and no output row more partials than this

inline int split_plan(long long bk, long long rows, long long Nmax, long long unit, int D, Plan* p) {
  long long want = 1;
  if (bk < kTargetWorkgroups && Nmax > kMinChunk) {
    want = (kTargetWorkgroups + bk - 1) / bk;
    if (want > Nmax / kMinChunk) want = Nmax / kMinChunk;
    if (want > kMaxSplits) want = kMaxSplits;
  }
  const long long chunk = ((Nmax + want - 1) / want + unit - 1) / unit * unit;
  const long long splits = (Nmax + chunk - 1) / chunk;
  if (chunk > 0x7fffffffLL || rows > 0x7fffffffLL || !grid_fits(bk * splits, rows, D)) return CLN_ERR_UNSUPPORTED;
  p->splits = (int)splits, p->chunk = (int)chunk;
  p->ws_bytes = workspace_bytes(rows, p->splits, D);
  return CLN_OK;
}

// the shape of a paged cache with grouped query heads: G = Hq / Hkv in {1, 2, 4, 8}, page a power of two in 16 .. 256, max_pages page an int
struct PagedGeometry {
  int group, g_shift, page_shift;
  long long Nmax;
};
inline int paged_geometry(int Hq, int Hkv, int max_pages, int page, PagedGeometry* g) {
  if (Hq <= 0 || Hkv <= 0 || max_pages <= 0 || page <= 0 || Hq % Hkv != 0) return CLN_ERR_BAD_ARG;
  g->group = Hq / Hkv;
  g->g_shift = g->group == 1 ? 0 : g->group == 2 ? 1 : g->group == 4 ? 2 : 3;
  if ((1 << g->g_shift) != g->group) return CLN_ERR_UNSUPPORTED;
  g->page_shift = 0;
  while ((1 << g->page_shift) < page && g->page_shift < 9) ++g->page_shift;
  if ((1 << g->page_shift) != page || page < 16 || page > 256) return CLN_ERR_UNSUPPORTED;
  g->Nmax = (long long)max_pages * page;
  return g->Nmax > 0x7fffffffLL ? CLN_ERR_UNSUPPORTED : CLN_OK;
}

// the out-parameters of a *_plan entry, each of which may be null
inline int plan_out(int rc, const Plan& p, int* splits, int* chunk, long long* ws_bytes) {
  if (rc != CLN_OK) return rc;
  if (splits) *splits = p.splits;
  if (chunk) *chunk = p.chunk;
  if (ws_bytes) *ws_bytes = p.ws_bytes;
  return CLN_OK;
}

// The pointers of an entry: n_in inputs, all required, 16-byte aligned up to first_int and 4-byte aligned from there on (the int32 arrays);
// out = {o, lse, workspace}, 16-byte aligned, lse and workspace may be null, and no output is an input or another output.
inline int check_pointers(const void* const* in, int n_in, int first_int, const void* const (&out)[3]) {
  for (int i = 0; i < n_in; ++i)
    if (!in[i] || !cln_aligned(in[i], i >= first_int ? 4 : 16)) return CLN_ERR_BAD_ARG;
  if (!out[0]) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 3; ++i) {
    if (!out[i]) continue;
    if (!cln_aligned16(out[i])) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < n_in; ++j)
      if (out[i] == in[j]) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < i; ++j)
      if (out[i] == out[j]) return CLN_ERR_BAD_ARG;
  }
  return CLN_OK;
}
inline bool workspace_fits(const Plan& p, const void* workspace, long long bytes) { return p.splits == 1 || (workspace && bytes >= p.ws_bytes); }

// the end of a describe text behind the n characters of the stream kernel's part; `row` names what the splits are merged for
inline int describe_tail(char* buf, int len, int n, const Plan& p, int D, const char* row, const char* last) {
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n, "; then fa2_decode_combine<D=%d> merges the live splits of a %s by log-sum-exp in ascending order (workspace %lld bytes)",
                  D, row, p.ws_bytes);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic%s", last);
  return n < len ? n : len - 1;
}

}  // namespace fa2d
