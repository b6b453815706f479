// Compile unit of the activation quantiser of the MXFP4-weight GEMMs: cln_quant_mxfp8_bf16 / cln_quant_mxfp8_bf16_describe
// (include/cln_amd_ext.h; kernel: quant_mxfp8_bf16.cuh). Status: -2 for M < 1, K < 32, K % 32 != 0 or a shape past one launch;
// then -1 for a missing, misaligned (x, codes 16 bytes) or aliased pointer.
#include "quant_mxfp8_bf16.cuh"

namespace qmx {
__global__ __launch_bounds__(kva::kThreads) void quant_mxfp8_bf16_rows(const Args a) {
  const unsigned long long u = (unsigned long long)blockIdx.x * kva::kThreads + threadIdx.x;
  const unsigned long long blk = u >> 2;
  const unsigned j = (unsigned)u & 3u;
  if (blk >= (unsigned long long)a.blocks) return;
  quant_piece(a.x + blk * 32u + 8u * j, a.codes + blk * 32u + 8u * j, a.scales + blk, j);
}
}  // namespace qmx

static int quant_shape(int M, int K, long long* blocks, long long* wgs) {
  if (M < 1 || K < 32 || K % 32) return CLN_ERR_UNSUPPORTED;
  *blocks = (long long)M * (K / 32);
  *wgs = qmx::workgroups(*blocks);
  return *wgs ? CLN_OK : CLN_ERR_UNSUPPORTED;
}

CLN_API int cln_quant_mxfp8_bf16(const void* x, void* codes, void* scales, int M, int K, void* stream) {
  long long blocks = 0, wgs = 0;
  const int rc = quant_shape(M, K, &blocks, &wgs);
  if (rc != CLN_OK) return rc;
  if (!x || !codes || !scales || !cln_aligned16(x) || !cln_aligned16(codes)) return CLN_ERR_BAD_ARG;
  if (x == codes || x == scales || codes == scales) return CLN_ERR_BAD_ARG;
  const qmx::Args a = {(const bf16_t*)x, (uint8_t*)codes, (uint8_t*)scales, blocks};
  CLN_LAUNCH(qmx::quant_mxfp8_bf16_rows, dim3((unsigned)wgs), dim3(kva::kThreads), 0, (hipStream_t)stream, a);
  return cln_check_launch();
}

CLN_API int cln_quant_mxfp8_bf16_describe(int M, int K, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  long long blocks = 0, wgs = 0;
  const int rc = quant_shape(M, K, &blocks, &wgs);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "quant_mxfp8_bf16_rows M=%d K=%d: one launch, no workspace, no LDS, no atomics, 0 bytes scratch, no spill; %lld workgroups "
                         "of 256 threads over %lld MX blocks of 32 columns (4 threads a block: 16 bytes in, 8 bytes out a thread); per block E = "
                         "the exponent field of fp32(amax |x|), scale byte = clamp(E - 8, 0, 254) (e8m0, the OCP MX floor rule with emax 8), inv = "
                         "2^(127 - scale) on its bits, code = e4m3fn rne of clamp(x inv, -448, 448); the amax over the 4 lanes of a block by two DPP "
                         "moves (the lanes of a block leave or stay together), lane 0 stores the scale byte [M, K/32]; deterministic",
                         M, K, wgs, blocks);
  return n < len ? n : len - 1;
}
