// Compile unit of the activation quantiser of the block-scaled FP8 GEMM: cln_quant_fp8_block128_bf16 / cln_quant_fp8_block128_bf16_describe
// (include/cln_amd_ext.h; kernel: quant_fp8_block128_bf16.cuh). Status: -2 for M < 1, K < 128, K % 128 != 0 or a shape past one
// launch; then -1 for a missing, misaligned (16 bytes; scales 4) or aliased pointer or a scale_pow2 that is neither 0 nor 1.
#include "quant_fp8_block128_bf16.cuh"

namespace q8 {
__global__ __launch_bounds__(kva::kThreads) void quant_fp8_block128_bf16_rows(const Args a) {
  const unsigned long long u = (unsigned long long)blockIdx.x * kva::kThreads + threadIdx.x;
  const unsigned long long blk = u >> 4;
  const unsigned j = (unsigned)u & 15u;
  if (blk >= (unsigned long long)a.blocks) return;
  quant_piece(a.x + blk * 128u + 8u * j, a.codes + blk * 128u + 8u * j, a.scales + blk, j, a.pow2);
}
}  // namespace q8

static int quant_shape(int M, int K, long long* blocks, long long* wgs) {
  if (M < 1 || K < 128 || K % 128) return CLN_ERR_UNSUPPORTED;
  *blocks = (long long)M * (K / 128);
  *wgs = q8::workgroups(*blocks);
  return *wgs ? CLN_OK : CLN_ERR_UNSUPPORTED;
}

CLN_API int cln_quant_fp8_block128_bf16(const void* x, void* codes, float* scales, int M, int K, int scale_pow2, void* stream) {
  long long blocks = 0, wgs = 0;
  const int rc = quant_shape(M, K, &blocks, &wgs);
  if (rc != CLN_OK) return rc;
  if (!x || !codes || !scales || !cln_aligned16(x) || !cln_aligned16(codes) || !cln_aligned(scales, 4)) return CLN_ERR_BAD_ARG;
  if (x == codes || x == (const void*)scales || codes == (void*)scales) return CLN_ERR_BAD_ARG;
  if (scale_pow2 != 0 && scale_pow2 != 1) return CLN_ERR_BAD_ARG;
  const q8::Args a = {(const bf16_t*)x, (uint8_t*)codes, scales, blocks, scale_pow2};
  CLN_LAUNCH(q8::quant_fp8_block128_bf16_rows, dim3((unsigned)wgs), dim3(kva::kThreads), 0, (hipStream_t)stream, a);
  return cln_check_launch();
}

CLN_API int cln_quant_fp8_block128_bf16_describe(int M, int K, int scale_pow2, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  long long blocks = 0, wgs = 0;
  const int rc = quant_shape(M, K, &blocks, &wgs);
  if (rc != CLN_OK) return rc;
  if (scale_pow2 != 0 && scale_pow2 != 1) return CLN_ERR_BAD_ARG;
  const int n = snprintf(buf, len,
                         "quant_fp8_block128_bf16_rows M=%d K=%d scale_pow2=%d: one launch, no workspace, no LDS, no atomics, 0 bytes scratch; %lld "
                         "workgroups of 256 threads over %lld blocks of 128 columns (16 threads a block: 16 bytes in, 8 bytes out a thread); per "
                         "block in IEEE fp32 a = max(amax, 1e-4), scale = a / 448%s, inv = 1 / scale, code = e4m3fn rne of clamp(x inv, -448, "
                         "448); the amax over the 16 lanes of a block by four DPP moves (the lanes of a block leave or stay together), lane 0 "
                         "stores the scale [M, K/128]; deterministic",
                         M, K, scale_pow2, wgs, blocks, scale_pow2 ? " rounded up to a power of two on its bits (ue8m0)" : "");
  return n < len ? n : len - 1;
}
