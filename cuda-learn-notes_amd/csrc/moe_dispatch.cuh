// The quantising dispatch of a mixture-of-experts layer (cln_moe_dispatch_fp8_block128_bf16, cln_moe_dispatch_mxfp8_bf16,
// include/cln_amd_ext.h): x bf16 [T, K] and src int32 [rows] (cln_moe_sort's: sorted row -> slot t k + j) -> codes [rows, K]
// and scales [rows, K / 128] (fp32) or [rows, K / 32] (e8m0 bytes). Row r carries the bits that the quantiser gives for row src[r] / k of x: the
// per-block arithmetic is q8::quant_piece / qmx::quant_piece, called and not copied. A row whose src is outside [0, T k) is not written; the test
// is made here, on the device, so a malformed list addresses nothing outside x.
//
// What is new is the row map. A row is 1 << sh thread places of 8 columns (the first K / 8 of them live), a workgroup of 256 threads covers
// 256 >> sh whole rows (sh < 8) or a 256-place piece of one row (blockIdx.y the piece): src[r] is loaded once per row -- one address for all
// lanes that share the row -- and a row's lanes leave or stay together, so the quantisers' DPP groups (16 or 4 consecutive lanes) are whole.
// 2 K bytes read and K + scales written per live row, in one launch; no LDS, no atomics.
#pragma once
#include "quant_fp8_block128_bf16.cuh"
#include "quant_mxfp8_bf16.cuh"

namespace moe {

struct DispatchArgs {
  const bf16_t* x;
  const int* src;
  uint8_t* codes;
  void* scales;
  int rows, T, k, K, sh, pow2;
};

template <bool MX>
__global__ __launch_bounds__(kva::kThreads) void moe_dispatch_rows(const DispatchArgs a) {
  const unsigned place = blockIdx.y * kva::kThreads + threadIdx.x;
  const unsigned r = blockIdx.x * (a.sh < 8 ? kva::kThreads >> a.sh : 1u) + (place >> a.sh);
  const unsigned col = 8u * (place & ((1u << a.sh) - 1u));
  if (r >= (unsigned)a.rows || col >= (unsigned)a.K) return;  // whole DPP groups: K is a multiple of the block
  const unsigned s = (unsigned)a.src[r];
  if (s >= (unsigned)a.T * (unsigned)a.k) return;  // a dropped row: all its lanes
  const bf16_t* x8 = a.x + (size_t)(s / (unsigned)a.k) * a.K + col;
  uint8_t* c8 = a.codes + (size_t)r * a.K + col;
  if constexpr (MX) qmx::quant_piece(x8, c8, (uint8_t*)a.scales + (size_t)r * (a.K / 32) + col / 32, (col / 8) & 3u);
  else q8::quant_piece(x8, c8, (float*)a.scales + (size_t)r * (a.K / 128) + col / 128, (col / 8) & 15u, a.pow2);
}

}  // namespace moe
