// Compile unit of the causal attention entry cln_fa2_fwd_causal (include/cln_amd_ext.h; kernel: flash_attn_causal.cuh). Built with
// -fno-slp-vectorize for the reason flash_attn_m16x.hip states: hipcc's SLP pass pairs the per-score f32 row-sum adds into v_pk_add_f32,
// which drags the exponentials of a whole phase behind its last MFMA.
#include "flash_attn_causal.cuh"
#include <stdio.h>
#include <string.h>

namespace {

// heaviest row blocks first, heads still pinned to XCDs (profiles/r07_fa_causal_bench.log: the three orders at [2,32,4096,128])
constexpr int kCausalOrder = fa2::M16X_ORDER_HEAVY;

struct CausalPlan {
  int rc;
  bool one_stage;
};

// the checks of the launch and of cln_describe: no device access
CausalPlan causal_plan(int B, int H, int N, int D, int stages) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return {CLN_ERR_BAD_ARG, false};
  if (D != 64 && D != 128) return {CLN_ERR_UNSUPPORTED, false};
  if (N % 256 != 0) return {CLN_ERR_UNSUPPORTED, false};  // 256-row workgroups (8 waves x 32 rows)
  if ((long long)B * H * (long long)(N / 256) > 0x7fffffffLL) return {CLN_ERR_UNSUPPORTED, false};  // grid size (x)
  return {CLN_OK, stages == 1};
}

}  // namespace

CLN_API int cln_fa2_fwd_causal(const void* q, const void* k, const void* v, void* o, int B, int H, int N, int D, int stages, void* stream) {
  if (!q || !k || !v || !o) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(q) || !cln_aligned16(k) || !cln_aligned16(v) || !cln_aligned16(o)) return CLN_ERR_BAD_ARG;
  const CausalPlan p = causal_plan(B, H, N, D, stages);
  if (p.rc != CLN_OK) return p.rc;
  return fa2c::run_causal<kCausalOrder>(D, p.one_stage, q, k, v, o, B, H, N, (hipStream_t)stream);
}

// describe hook (cln_describe, describe.hip): CLN_ERR_BAD_ARG when `name` is not the causal entry
int cln_fa_causal_describe(const char* name, int B, int H, int N, int D, int stages, char* buf, int len) {
  if (strcmp(name, "cln_fa2_fwd_causal") != 0) return CLN_ERR_BAD_ARG;
  const CausalPlan p = causal_plan(B, H, N, D, stages);
  if (p.rc != CLN_OK) return p.rc;
  return snprintf(buf, len, "fa2_fwd_m16x_causal<D=%d,BC=128,16x16x32 MFMA,pre-scaled Q,sum-checked softmax,key <= query> 8 waves x 32 rows, "
                            "two groups one phase apart, row block qb runs 2(qb+1) key tiles, masked on the last two, heaviest row blocks first%s",
                  D, p.one_stage ? " [single stage: every tile fetch waited for where it is issued]" : "");
}
