// Compile unit of the MoE weighted combine: cln_moe_combine_bf16 / cln_moe_combine_bf16_describe (include/cln_amd_ext.h; kernel:
// moe_combine.cuh). Status, in this order: a non-positive M_total, T, N or k (-1); N % 8 != 0, k > 16 or N > 2^22 (-2); a
// missing pointer (residual may be null), y, out or residual not 16-byte aligned, pos or the weights not 4-byte aligned, out equal to an
// input (-1).
#include "moe_combine.cuh"

struct CombinePlan {
  unsigned gy, threads;
};

static int combine_plan(int M, int T, int N, int k, CombinePlan* p) {
  if (M < 1 || T < 1 || N < 1 || k < 1) return CLN_ERR_BAD_ARG;
  if (N % 8 || k > moe::kCombineMaxK || N > (1 << 22)) return CLN_ERR_UNSUPPORTED;
  const unsigned pieces = (unsigned)N / 8;
  p->gy = (pieces + 255) / 256;
  p->threads = ((pieces + p->gy - 1) / p->gy + 63) / 64 * 64;
  return CLN_OK;
}

CLN_API int cln_moe_combine_bf16(const void* y, const int* pos, const float* topk_weights, const void* residual, void* out, int M_total, int T,
                                 int N, int k, void* stream) {
  CombinePlan p;
  const int rc = combine_plan(M_total, T, N, k, &p);
  if (rc != CLN_OK) return rc;
  if (!y || !pos || !topk_weights || !out || !cln_aligned16(y) || !cln_aligned16(out) || !cln_aligned16(residual) || !cln_aligned(pos, 4) ||
      !cln_aligned(topk_weights, 4))
    return CLN_ERR_BAD_ARG;
  if (out == y || out == residual || out == (const void*)pos || out == (const void*)topk_weights) return CLN_ERR_BAD_ARG;
  const moe::CombineArgs a = {(const bf16_t*)y, (const bf16_t*)residual, pos, topk_weights, (bf16_t*)out, M_total, N, k};
  CLN_LAUNCH(moe::moe_combine_rows, dim3((unsigned)T, p.gy), dim3(p.threads), 0, (hipStream_t)stream, a);
  return cln_check_launch();
}

CLN_API int cln_moe_combine_bf16_describe(int M_total, int T, int N, int k, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  CombinePlan p;
  const int rc = combine_plan(M_total, T, N, k, &p);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "moe_combine_rows M_total=%d T=%d N=%d k=%d: one launch, no workspace, 128 bytes LDS static, no atomics, 0 bytes scratch, no "
                         "spill; grid %d x %u workgroups of %u threads (a token, a run of column pieces), a thread owns 8 columns and loads 16 "
                         "bytes a term; the k positions and weights of the token are loaded once per workgroup into LDS, the row loads are issued "
                         "before the first fmaf; out = bf16 rne of residual + sum_j w_j y[pos_j] in fp32, one fmaf a term in ascending j; a pos "
                         "outside [0, M_total) contributes nothing; deterministic",
                         M_total, T, N, k, T, p.gy, p.threads);
  return n < len ? n : len - 1;
}
