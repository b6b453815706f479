// Compile unit of the attention backward entries cln_fa2_bwd / cln_fa2_bwd_causal (include/cln_amd_ext.h; kernels: flash_attn_bwd.cuh).
// Built with -fno-slp-vectorize, as the forward units: hipcc's SLP pass would pair the per-score f32 multiplies into v_pk_mul_f32.
#include "flash_attn_bwd.cuh"
#include <stdio.h>
#include <string.h>

namespace {

// the checks of the launch and of cln_describe: no device access
int bwd_plan(int B, int H, int N, int D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  if (N % 256 != 0) return CLN_ERR_UNSUPPORTED;
  if ((long long)B * H * (long long)(N / 128) > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;  // grid size (x): 128-row blocks
  return CLN_OK;
}

int bwd_entry(bool causal, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta,
              void* dq, void* dk, void* dv, int B, int H, int N, int D, void* stream) {
  const void* in[] = {q, k, v, o, dout, lse};
  const void* out[] = {delta, dq, dk, dv};
  for (const void* p : in)
    if (!p || !cln_aligned16(p)) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 4; ++i) {
    if (!out[i] || !cln_aligned16(out[i])) return CLN_ERR_BAD_ARG;
    for (const void* p : in)
      if (out[i] == p) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < i; ++j)
      if (out[i] == out[j]) return CLN_ERR_BAD_ARG;
  }
  const int rc = bwd_plan(B, H, N, D);
  if (rc != CLN_OK) return rc;
  const hipStream_t s = (hipStream_t)stream;
  if (D == 64)
    return causal ? fa2b::launch_bwd<64, true>(q, k, v, o, dout, lse, delta, dq, dk, dv, B, H, N, s)
                  : fa2b::launch_bwd<64, false>(q, k, v, o, dout, lse, delta, dq, dk, dv, B, H, N, s);
  return causal ? fa2b::launch_bwd<128, true>(q, k, v, o, dout, lse, delta, dq, dk, dv, B, H, N, s)
                : fa2b::launch_bwd<128, false>(q, k, v, o, dout, lse, delta, dq, dk, dv, B, H, N, s);
}

}  // namespace

CLN_API int cln_fa2_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta,
                        void* dq, void* dk, void* dv, int B, int H, int N, int D, void* stream) {
  return bwd_entry(false, q, k, v, o, dout, lse, delta, dq, dk, dv, B, H, N, D, stream);
}

CLN_API int cln_fa2_bwd_causal(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta,
                               void* dq, void* dk, void* dv, int B, int H, int N, int D, void* stream) {
  return bwd_entry(true, q, k, v, o, dout, lse, delta, dq, dk, dv, B, H, N, D, stream);
}

// describe hook (cln_describe, describe.hip): CLN_ERR_BAD_ARG when `name` is not one of the two entries
int cln_fa_bwd_describe(const char* name, int B, int H, int N, int D, int stages, char* buf, int len) {
  (void)stages;
  const bool causal = strcmp(name, "cln_fa2_bwd_causal") == 0;
  if (!causal && strcmp(name, "cln_fa2_bwd") != 0) return CLN_ERR_BAD_ARG;
  const int rc = bwd_plan(B, H, N, D);
  if (rc != CLN_OK) return rc;
  return snprintf(buf, len, "fa2_bwd_dq<D=%d,16x16x32 MFMA%s> 4 waves x 32 query rows, delta then dQ over 64-key tiles%s; "
                            "then fa2_bwd_dkdv<D=%d,16x16x32 MFMA%s> 4 waves x 32 keys, dK and dV over 64-row query tiles%s; "
                            "deterministic [one pipeline: stages ignored]",
                  D, causal ? ",key <= query" : "", causal ? ", heaviest query blocks first" : "", D, causal ? ",key <= query" : "",
                  causal ? ", heaviest key blocks first" : "");
}
