// What the bf16 entries of the paged KV-cache path share (cln_kv_append_paged_varlen_bf16, cln_fa2_prefill_paged_varlen_bf16,
// cln_fa2_decode_paged_multi_bf16; include/cln_amd_ext.h): the element type, named HERE ONCE -- the vector types, the MFMA, the
// transposing LDS read, the paged cache and the output -- so that the three kernel bodies (siblings of the fp16 ones, which stay untouched: a
// shared body with a policy parameter cost the fp16 kernels up to 6 %, commit f5e8c73) speak of b8 / b4 / bf16_t only. Everything that knows no
// element type comes from flash_attn_decode_common.cuh by inclusion: paged_geometry, Split, split_of, Plan, split_plan, swap_pair, ex2, merge,
// reduce_waves, scale_log2, the workspace layout and the pointer checks.
//
// Numerics: K, V and q are bf16 operands of v_mfma_f32_16x16x32_bf16, scores and accumulators fp32; P is rounded once to bf16, round to nearest
// even (v_cvt_pk_bf16_f32), O once at the store. No value passes through fp16.
//
// No kernel name here ends in _kernel: tests/decode_kernels.py and the fp16 surface tests count those by the fp16 describe texts.
#pragma once
#include "flash_attn_decode_common.cuh"

typedef __bf16 bf16_t;
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));

namespace fa2b {

using fa2d::kThreads;
using fa2d::kWaves;

// c + a b on the matrix pipe; the operands stay alive across it (cln_mfma_keep, common.h)
__device__ __forceinline__ f4 mfma(const b8& a, const b8& b, f4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  cln_mfma_keep(c, a, b);
  return c;
}

// ds_read_b64_tr_b16 does not care what the 16 bits mean
__device__ __forceinline__ b4 lds_read_tr(const void* lds_addr) { return __builtin_bit_cast(b4, lds_read_tr16(lds_addr)); }
__device__ __forceinline__ b8 b8_cat(b4 lo, b4 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ b4 round4(const f4& x) { return b4{(bf16_t)x[0], (bf16_t)x[1], (bf16_t)x[2], (bf16_t)x[3]}; }

// fa2d::PagedKV with bf16 pools [P,Hkv,page,D]: the same table walk, the same index arithmetic (`off` in elements)
struct PagedKV {
  const bf16_t *k, *v;
  const int* table;
  int Hkv, max_pages, page_shift;
  __host__ __device__ int heads() const { return Hkv; }
  __host__ __device__ int nmax() const { return max_pages << page_shift; }  // the plan checked that it fits
  struct At {
    const bf16_t *k, *v;
    const int* bt;
    unsigned kvh, lo;
    int off;
  };
  __device__ At at(const fa2d::Split& w, int, int off) const { return {k, v, table + (size_t)w.b * max_pages, w.h, (unsigned)w.lo, off}; }
  // the physical page of row r; rows at or past n have no table entry that is ours to read
  __device__ int lookup(const At& a, unsigned r, unsigned n) const { return r < n ? a.bt[(a.lo + r) >> page_shift] : 0; }
  __device__ size_t elem(const At& a, int pg, unsigned r, int D) const {
    return ((((size_t)pg * Hkv + a.kvh) << page_shift) + ((a.lo + r) & ((1u << page_shift) - 1u))) * D + a.off;
  }
};

// fa2d::Out with a bf16 o [rows][D]; lse and the workspace (layout: flash_attn_decode_common.cuh) stay fp32
struct Out {
  bf16_t* o;
  float *lse, *ws_o, *ws_ml;
};
inline Out make_out(void* o, float* lse, void* workspace, long long rows, int S, int D) {
  float* ws = (float*)workspace;
  return {(bf16_t*)o, lse, ws, S > 1 ? ws + (size_t)rows * S * D : nullptr};
}

// fa2d::store_final / store_split with one rounding to bf16 at the store
template <int D>
__device__ __forceinline__ void store_final(const Out& out, size_t row, int t, float mx, float L, float O) {
  const float inv = L > 0.0f ? 1.0f / L : 0.0f;
  out.o[row * D + t] = (bf16_t)(O * inv);
  if (out.lse && t == 0) out.lse[row] = L > 0.0f ? (mx + __builtin_log2f(L)) * 0.6931471805599453f : FA2D_NEG_INF;
}
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

// fa2d::fa2_decode_combine_kernel storing bf16: the live splits ceil(len_b / C) of a row merged in ascending s, the same -inf guard
template <int D>
__global__ __launch_bounds__(D) void fa2_decode_combine_bf16_rows(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                                  const int* __restrict__ seqlens, bf16_t* __restrict__ o, float* __restrict__ lse,
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
    const float f = fa2d::ex2(ml[2 * s] - ms);
    L = fmaf(ml[2 * s + 1], f, L);
    O = fmaf(po[(size_t)s * D], f, O);
  }
  store_final<D>(Out{o, lse, nullptr, nullptr}, row, t, mx, L, O);
}

// the status of the stream kernel's launch, then for S > 1 the combine over `rows` output rows
template <int D>
int launch_combine(int rc, const Out& out, const int* seqlens, long long rows, int rows_per_seq, int Nmax, int S, int C, hipStream_t stream) {
  if (rc != CLN_OK || S == 1) return rc;
  CLN_LAUNCH((fa2_decode_combine_bf16_rows<D>), dim3((unsigned)rows), dim3(D), 0, stream, (const float*)out.ws_o, (const float*)out.ws_ml, seqlens,
             out.o, out.lse, rows_per_seq, Nmax, S, C);
  return cln_check_launch();
}

}  // namespace fa2b
