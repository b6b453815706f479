// Compile unit of the attention entries beyond the reference surface that run the sum-checked optimistic-softmax kernel of
// flash_attn_m16x.cuh (include/cln_amd_ext.h): cln_fa2_fwd_causal (CAUSAL = true) and the forwards that also write the row log-sum-exp,
// cln_fa2_fwd_lse / cln_fa2_fwd_causal_lse (LSE = true): the input of the backward (flash_attn_bwd.hip). Built with -fno-slp-vectorize
// for the reason flash_attn_m16x.hip states: hipcc's SLP pass pairs the per-score f32 row-sum adds into v_pk_add_f32, which drags the
// exponentials of a whole phase behind its last MFMA.
#include "flash_attn_m16x.cuh"
#include <stdio.h>
#include <string.h>

namespace {

struct ExtPlan {
  int rc;
  bool one_stage;
};

// the checks of the launch and of cln_describe: no device access
ExtPlan ext_plan(int B, int H, int N, int D, int stages) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return {CLN_ERR_BAD_ARG, false};
  if (D != 64 && D != 128) return {CLN_ERR_UNSUPPORTED, false};
  if (N % 256 != 0) return {CLN_ERR_UNSUPPORTED, false};  // 256-row workgroups (8 waves x 32 rows)
  if ((long long)B * H * (long long)(N / 256) > 0x7fffffffLL) return {CLN_ERR_UNSUPPORTED, false};  // grid size (x)
  return {CLN_OK, stages == 1};
}

// The 32-rows-per-wave kernels with the options of the plain ones (stages = 2 / stages = 1). Launch order: the causal entries run the
// heaviest row blocks first, heads still pinned to XCDs (profiles/r07_fa_causal_bench.log: the three orders at [2,32,4096,128]).
template <bool CAUSAL, bool LSE>
int ext_run(int D, bool one_stage, const void* q, const void* k, const void* v, void* o, void* aux, int B, int H, int N, hipStream_t s) {
  constexpr int ORDER = CAUSAL ? fa2::M16X_ORDER_HEAVY : fa2::M16X_ORDER_PLAIN;
  return one_stage ? fa2::launch_m16x_shipped<fa2::M16X_SHIPPED_1STAGE, false, CAUSAL, ORDER, LSE>(D, 32, q, k, v, o, aux, B, H, N, s)
                   : fa2::launch_m16x_shipped<fa2::M16X_SHIPPED, false, CAUSAL, ORDER, LSE>(D, 32, q, k, v, o, aux, B, H, N, s);
}

// lse == nullptr: O only (the causal entry; the plain O-only forward belongs to the reference names, flash_attn_m16x.hip)
int ext_entry(bool causal, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int D, int stages, void* stream) {
  if (!q || !k || !v || !o) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(q) || !cln_aligned16(k) || !cln_aligned16(v) || !cln_aligned16(o) || !cln_aligned16(lse)) return CLN_ERR_BAD_ARG;
  if (lse) {  // the LSE entries: no output on an input or on the other output
    for (const void* out : {(const void*)o, (const void*)lse})
      if (out == q || out == k || out == v) return CLN_ERR_BAD_ARG;
    if ((const void*)o == (const void*)lse) return CLN_ERR_BAD_ARG;
  }
  const ExtPlan p = ext_plan(B, H, N, D, stages);
  if (p.rc != CLN_OK) return p.rc;
  hipStream_t s = (hipStream_t)stream;
  if (lse) return causal ? ext_run<true, true>(D, p.one_stage, q, k, v, o, lse, B, H, N, s) : ext_run<false, true>(D, p.one_stage, q, k, v, o, lse, B, H, N, s);
  return causal ? ext_run<true, false>(D, p.one_stage, q, k, v, o, nullptr, B, H, N, s) : CLN_ERR_BAD_ARG;
}

}  // namespace

CLN_API int cln_fa2_fwd_causal(const void* q, const void* k, const void* v, void* o, int B, int H, int N, int D, int stages, void* stream) {
  return ext_entry(true, q, k, v, o, nullptr, B, H, N, D, stages, stream);
}

CLN_API int cln_fa2_fwd_lse(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int D, int stages, void* stream) {
  if (!lse) return CLN_ERR_BAD_ARG;
  return ext_entry(false, q, k, v, o, lse, B, H, N, D, stages, stream);
}

CLN_API int cln_fa2_fwd_causal_lse(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int D, int stages, void* stream) {
  if (!lse) return CLN_ERR_BAD_ARG;
  return ext_entry(true, q, k, v, o, lse, B, H, N, D, stages, stream);
}

// describe hook (cln_describe, describe.hip): CLN_ERR_BAD_ARG when `name` is not one of the three entries
int cln_fa_m16x_ext_describe(const char* name, int B, int H, int N, int D, int stages, char* buf, int len) {
  const bool lse = strcmp(name, "cln_fa2_fwd_lse") == 0 || strcmp(name, "cln_fa2_fwd_causal_lse") == 0;
  const bool causal = strcmp(name, "cln_fa2_fwd_causal") == 0 || strcmp(name, "cln_fa2_fwd_causal_lse") == 0;
  if (!lse && !causal) return CLN_ERR_BAD_ARG;
  const ExtPlan p = ext_plan(B, H, N, D, stages);
  if (p.rc != CLN_OK) return p.rc;
  const char* single = p.one_stage ? " [single stage: every tile fetch waited for where it is issued]" : "";
  if (!lse)
    return snprintf(buf, len, "fa2_fwd_m16x_causal<D=%d,BC=128,16x16x32 MFMA,pre-scaled Q,sum-checked softmax,key <= query> 8 waves x 32 rows, "
                              "two groups one phase apart, row block qb runs 2(qb+1) key tiles, masked on the last two, heaviest row blocks first%s",
                    D, single);
  return snprintf(buf, len, "fa2_fwd_m16x_lse<D=%d,BC=128,16x16x32 MFMA,pre-scaled Q,sum-checked softmax%s> 8 waves x 32 rows, two groups one phase apart, "
                            "fp32 row log-sum-exp from the epilogue%s%s",
                  D, causal ? ",key <= query" : "", causal ? ", heaviest row blocks first" : "", single);
}
