// Compile unit of the MoE quantising dispatch: cln_moe_dispatch_fp8_block128_bf16, cln_moe_dispatch_mxfp8_bf16 and their describe entries
// (include/cln_amd_ext.h; kernel: moe_dispatch.cuh). Status, in this order: a non-positive rows, T, k or K (-1); K not a
// multiple of the block (128, 32), K > 2^20 or T k past 2^31 - 1 (-2); a missing, misaligned (x, codes 16 bytes;
// src, fp32 scales 4) or aliased pointer, a scale_pow2 that is neither 0 nor 1 (-1).
#include "moe_dispatch.cuh"

struct DispatchPlan {
  int sh;
  unsigned gx, gy;
};

static int dispatch_plan(int rows, int T, int k, int K, int block, DispatchPlan* p) {
  if (rows < 1 || T < 1 || k < 1 || K < 1) return CLN_ERR_BAD_ARG;
  if (K % block || K > (1 << 20) || (long long)T * k > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  p->sh = 2;
  while ((8 << p->sh) < K) ++p->sh;
  p->gy = p->sh < 8 ? 1u : 1u << (p->sh - 8);
  const int rpw = p->sh < 8 ? 256 >> p->sh : 1;
  p->gx = (unsigned)((rows + rpw - 1) / rpw);
  return CLN_OK;
}

static int dispatch(bool mx, const void* x, const int* src, void* codes, void* scales, int rows, int T, int k, int K, int pow2, void* stream) {
  DispatchPlan p;
  const int rc = dispatch_plan(rows, T, k, K, mx ? 32 : 128, &p);
  if (rc != CLN_OK) return rc;
  if (!x || !src || !codes || !scales || !cln_aligned16(x) || !cln_aligned16(codes) || !cln_aligned(src, 4) || !cln_aligned(scales, mx ? 1 : 4))
    return CLN_ERR_BAD_ARG;
  if (x == codes || x == scales || codes == scales || (const void*)src == codes || (const void*)src == scales) return CLN_ERR_BAD_ARG;
  if (pow2 != 0 && pow2 != 1) return CLN_ERR_BAD_ARG;
  const moe::DispatchArgs a = {(const bf16_t*)x, src, (uint8_t*)codes, scales, rows, T, k, K, p.sh, pow2};
  if (mx) CLN_LAUNCH(moe::moe_dispatch_rows<true>, dim3(p.gx, p.gy), dim3(kva::kThreads), 0, (hipStream_t)stream, a);
  else CLN_LAUNCH(moe::moe_dispatch_rows<false>, dim3(p.gx, p.gy), dim3(kva::kThreads), 0, (hipStream_t)stream, a);
  return cln_check_launch();
}

static int dispatch_describe(bool mx, int rows, int T, int k, int K, int pow2, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  DispatchPlan p;
  const int rc = dispatch_plan(rows, T, k, K, mx ? 32 : 128, &p);
  if (rc != CLN_OK) return rc;
  if (pow2 != 0 && pow2 != 1) return CLN_ERR_BAD_ARG;
  const int n = snprintf(buf, len,
                         "moe_dispatch_rows<%s> rows=%d T=%d k=%d K=%d%s: one launch, no workspace, no LDS, no atomics, 0 bytes scratch, no spill; grid "
                         "%u x %u workgroups of 256 threads, %d thread places of 8 columns a row (%d live), %d row(s) a workgroup; row r = the "
                         "bits of %s on row src[r] / k of x (its per-block rule by inclusion: %s), src[r] loaded once per row, a row with src "
                         "outside [0, T k) is not written (tested on the device); 16 bytes in, 8 bytes out a thread; deterministic",
                         mx ? "mxfp8" : "fp8_block128", rows, T, k, K, mx ? "" : (pow2 ? " scale_pow2=1" : " scale_pow2=0"), p.gx, p.gy, 1 << p.sh,
                         K / 8, p.sh < 8 ? 256 >> p.sh : 1, mx ? "quant_mxfp8_bf16" : "quant_fp8_block128_bf16",
                         mx ? "qmx::quant_piece, 4 lanes a block of 32" : "q8::quant_piece, 16 lanes a block of 128");
  return n < len ? n : len - 1;
}

CLN_API int cln_moe_dispatch_fp8_block128_bf16(const void* x, const int* src, void* codes, float* scales, int rows, int T, int k, int K,
                                               int scale_pow2, void* stream) {
  return dispatch(false, x, src, codes, scales, rows, T, k, K, scale_pow2, stream);
}
CLN_API int cln_moe_dispatch_fp8_block128_bf16_describe(int rows, int T, int k, int K, int scale_pow2, char* buf, int len) {
  return dispatch_describe(false, rows, T, k, K, scale_pow2, buf, len);
}
CLN_API int cln_moe_dispatch_mxfp8_bf16(const void* x, const int* src, void* codes, void* scales, int rows, int T, int k, int K, void* stream) {
  return dispatch(true, x, src, codes, scales, rows, T, k, K, 0, stream);
}
CLN_API int cln_moe_dispatch_mxfp8_bf16_describe(int rows, int T, int k, int K, char* buf, int len) {
  return dispatch_describe(true, rows, T, k, K, 0, buf, len);
}
