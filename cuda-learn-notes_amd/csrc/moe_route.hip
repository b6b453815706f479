// Compile unit of the MoE router: cln_moe_route_topk / cln_moe_route_topk_describe (include/cln_amd_ext.h; kernel: moe_route.cuh; DESIGN
// 4.4.33). Status, in this order: a non-positive T, E or k (-1); E > 512, k > min(E, 16), a scoring that is neither 0 nor 1, a bias with
// softmax (-2); a missing, misaligned (4 bytes; bf16 logits 2) or aliased pointer, a
// logits_fp32 or renormalize that is neither 0 nor 1 (-1).
#include "moe_route.cuh"

static int route_shape(int T, int E, int k, int scoring, int has_bias) {
  if (T < 1 || E < 1 || k < 1) return CLN_ERR_BAD_ARG;
  if (E > moe::kRouteMaxE || k > moe::kRouteMaxK || k > E) return CLN_ERR_UNSUPPORTED;
  if (scoring != moe::kSoftmax && scoring != moe::kSigmoid) return CLN_ERR_UNSUPPORTED;
  if (has_bias && scoring != moe::kSigmoid) return CLN_ERR_UNSUPPORTED;
  return CLN_OK;
}

static int route_regs(int E) { return E <= 64 ? 1 : E <= 128 ? 2 : E <= 256 ? 4 : 8; }

template <typename T>
static void route_launch(const moe::RouteArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.T + 3) / 4)), block(moe::kRouteThreads);
  switch (route_regs(a.E)) {
    case 1: CLN_LAUNCH((moe::moe_route_topk_wave<T, 1>), grid, block, 0, stream, a); break;
    case 2: CLN_LAUNCH((moe::moe_route_topk_wave<T, 2>), grid, block, 0, stream, a); break;
    case 4: CLN_LAUNCH((moe::moe_route_topk_wave<T, 4>), grid, block, 0, stream, a); break;
    default: CLN_LAUNCH((moe::moe_route_topk_wave<T, 8>), grid, block, 0, stream, a); break;
  }
}

CLN_API int cln_moe_route_topk(const void* logits, const float* bias, int* topk_ids, float* topk_weights, int T, int E, int k, int logits_fp32,
                               int scoring, int renormalize, float scale, void* stream) {
  const int rc = route_shape(T, E, k, scoring, bias != nullptr);
  if (rc != CLN_OK) return rc;
  if (!logits || !topk_ids || !topk_weights || (logits_fp32 != 0 && logits_fp32 != 1) || (renormalize != 0 && renormalize != 1)) return CLN_ERR_BAD_ARG;
  if (!cln_aligned(logits, logits_fp32 ? 4 : 2) || !cln_aligned(topk_ids, 4) || !cln_aligned(topk_weights, 4) || !cln_aligned(bias, 4))
    return CLN_ERR_BAD_ARG;
  if (logits == (const void*)topk_ids || logits == (const void*)topk_weights || (const void*)topk_ids == (const void*)topk_weights ||
      (bias && ((const void*)bias == (const void*)topk_ids || (const void*)bias == (const void*)topk_weights)))
    return CLN_ERR_BAD_ARG;
  const moe::RouteArgs a = {logits, bias, topk_ids, topk_weights, T, E, k, scoring, renormalize, scale};
  if (logits_fp32) route_launch<float>(a, (hipStream_t)stream);
  else route_launch<bf16_t>(a, (hipStream_t)stream);
  return cln_check_launch();
}

CLN_API int cln_moe_route_topk_describe(int T, int E, int k, int logits_fp32, int scoring, int renormalize, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  const int rc = route_shape(T, E, k, scoring, 0);
  if (rc != CLN_OK) return rc;
  if ((logits_fp32 != 0 && logits_fp32 != 1) || (renormalize != 0 && renormalize != 1)) return CLN_ERR_BAD_ARG;
  const int n = snprintf(buf, len,
                         "moe_route_topk_wave<%s, %d> T=%d E=%d k=%d %s%s: one launch, no workspace, no LDS, no atomics, 0 bytes scratch, no spill; "
                         "grid %d workgroups of 256 threads, one wave a token (4 tokens a workgroup), %d keys a lane in registers (expert 64 i + "
                         "lane); %d rounds of a wave-wide arg-max of (key, -index) over 4 DPP moves and 2 v_permlane swaps, the winning lane "
                         "retires its key, lane j keeps winner j; key = %s; weight = scale * %s; equal keys go to the lower index; finite "
                         "logits are the caller's contract; deterministic",
                         logits_fp32 ? "float" : "bf16", route_regs(E), T, E, k, scoring ? "sigmoid" : "softmax", renormalize ? " renormalize" : "",
                         (T + 3) / 4, route_regs(E), k, scoring ? "1 / (1 + exp(-l)) + bias in fp32" : "the logit (bf16 -> fp32 is exact)",
                         scoring ? (renormalize ? "s_j / sum of the selected s (s without the bias)" : "s_j (without the bias)")
                                 : (renormalize ? "exp(l_j - l_max) / sum over the selected" : "exp(l_j - l_max) / sum over all E"));
  return n < len ? n : len - 1;
}
