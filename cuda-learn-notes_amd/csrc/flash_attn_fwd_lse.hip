// Compile unit of the attention forwards that also write the row log-sum-exp, cln_fa2_fwd_lse / cln_fa2_fwd_causal_lse
// (include/cln_amd_ext.h): the input of the backward (flash_attn_bwd.hip). The kernel is the 32-rows-per-wave sum-checked
// optimistic-softmax body of flash_attn_m16x.cuh with LSE = true, in its own namespace and unit so the plain (fa2::) and causal
// (fa2c::) kernel sets and their instruction streams stay as they are. Built with -fno-slp-vectorize for the reason
// flash_attn_m16x.hip states: hipcc's SLP pass pairs the per-score f32 row-sum adds into v_pk_add_f32, which drags the
// exponentials of a whole phase behind its last MFMA.
#include "flash_attn_causal.cuh"
#include <stdio.h>
#include <string.h>

namespace fa2b {
using namespace fa2;

template <int D_, int PD, int NDEF, int OX, bool CAUSAL_, int ORDER>
__global__ __launch_bounds__(512, 2) void fa2_fwd_m16x_lse_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K,
                                                                  const half_t* __restrict__ V, half_t* __restrict__ O, float* __restrict__ lse,
                                                                  int N, int n_qblk, int n_heads, float scale_log2e) {
  constexpr int RPW_ = 32, BC_ = 128;
  constexpr bool VT = false, CAUSAL = CAUSAL_, LSE = true;
  [[maybe_unused]] unsigned long long* stamps = nullptr;
#include "flash_attn_m16x_body.inc"
}

template <int D_, int PD, int NDEF, int OX, bool CAUSAL>
int launch_lse(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, hipStream_t stream) {
  using G = GeoM16<D_, 32, 128>;
  constexpr int ORDER = CAUSAL ? M16X_ORDER_HEAVY : M16X_ORDER_PLAIN;  // the orders of the causal and the plain entries
  if (N % G::BR != 0) return CLN_ERR_UNSUPPORTED;
  static cln_lds_attr lds_attr;  // per device, thread-safe (common.h)
  if (cln_ensure_lds(lds_attr, reinterpret_cast<const void*>(&fa2_fwd_m16x_lse_kernel<D_, PD, NDEF, OX, CAUSAL, ORDER>), G::LDS_BYTES) != CLN_OK) return CLN_ERR_LAUNCH;
  const float scale_log2e = 1.4426950408889634f / sqrtf((float)G::D);
  const int n_qblk = N / G::BR;
  CLN_LAUNCH((fa2_fwd_m16x_lse_kernel<D_, PD, NDEF, OX, CAUSAL, ORDER>), dim3(n_qblk * B * H), dim3(G::NT), G::LDS_BYTES, stream,
             (const half_t*)q, (const half_t*)k, (const half_t*)v, (half_t*)o, lse, N, n_qblk, B * H, scale_log2e);
  return cln_check_launch();
}

// the options of the 32-rows-per-wave plain and causal kernels (stages = 2 / stages = 1): the same O bits as those
template <bool CAUSAL>
int run_lse(int D, bool one_stage, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, hipStream_t s) {
  constexpr int OX = fa2c::CAUSAL_OX, O1 = fa2c::CAUSAL_O1;
  if (D == 64) return one_stage ? launch_lse<64, 8, 4, O1, CAUSAL>(q, k, v, o, lse, B, H, N, s) : launch_lse<64, 8, 4, OX, CAUSAL>(q, k, v, o, lse, B, H, N, s);
  if (D == 128) return one_stage ? launch_lse<128, 4, 4, O1, CAUSAL>(q, k, v, o, lse, B, H, N, s) : launch_lse<128, 4, 4, OX, CAUSAL>(q, k, v, o, lse, B, H, N, s);
  return CLN_ERR_UNSUPPORTED;
}

}  // namespace fa2b

namespace {

struct LsePlan {
  int rc;
  bool one_stage;
};

// the checks of the launch and of cln_describe: no device access
LsePlan lse_plan(int B, int H, int N, int D, int stages) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return {CLN_ERR_BAD_ARG, false};
  if (D != 64 && D != 128) return {CLN_ERR_UNSUPPORTED, false};
  if (N % 256 != 0) return {CLN_ERR_UNSUPPORTED, false};  // 256-row workgroups (8 waves x 32 rows)
  if ((long long)B * H * (long long)(N / 256) > 0x7fffffffLL) return {CLN_ERR_UNSUPPORTED, false};  // grid size (x)
  return {CLN_OK, stages == 1};
}

int lse_entry(bool causal, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int D, int stages, void* stream) {
  if (!q || !k || !v || !o || !lse) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(q) || !cln_aligned16(k) || !cln_aligned16(v) || !cln_aligned16(o) || !cln_aligned16(lse)) return CLN_ERR_BAD_ARG;
  for (const void* out : {(const void*)o, (const void*)lse})
    if (out == q || out == k || out == v) return CLN_ERR_BAD_ARG;
  if ((const void*)o == (const void*)lse) return CLN_ERR_BAD_ARG;
  const LsePlan p = lse_plan(B, H, N, D, stages);
  if (p.rc != CLN_OK) return p.rc;
  return causal ? fa2b::run_lse<true>(D, p.one_stage, q, k, v, o, lse, B, H, N, (hipStream_t)stream)
                : fa2b::run_lse<false>(D, p.one_stage, q, k, v, o, lse, B, H, N, (hipStream_t)stream);
}

}  // namespace

CLN_API int cln_fa2_fwd_lse(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int D, int stages, void* stream) {
  return lse_entry(false, q, k, v, o, lse, B, H, N, D, stages, stream);
}

CLN_API int cln_fa2_fwd_causal_lse(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int D, int stages, void* stream) {
  return lse_entry(true, q, k, v, o, lse, B, H, N, D, stages, stream);
}

// describe hook (cln_describe, describe.hip): CLN_ERR_BAD_ARG when `name` is not one of the two entries
int cln_fa_lse_describe(const char* name, int B, int H, int N, int D, int stages, char* buf, int len) {
  const bool causal = strcmp(name, "cln_fa2_fwd_causal_lse") == 0;
  if (!causal && strcmp(name, "cln_fa2_fwd_lse") != 0) return CLN_ERR_BAD_ARG;
  const LsePlan p = lse_plan(B, H, N, D, stages);
  if (p.rc != CLN_OK) return p.rc;
  return snprintf(buf, len, "fa2_fwd_m16x_lse<D=%d,BC=128,16x16x32 MFMA,pre-scaled Q,sum-checked softmax%s> 8 waves x 32 rows, two groups one phase apart, "
                            "fp32 row log-sum-exp from the epilogue%s%s",
                  D, causal ? ",key <= query" : "", causal ? ", heaviest row blocks first" : "",
                  p.one_stage ? " [single stage: every tile fetch waited for where it is issued]" : "");
}
