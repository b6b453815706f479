// Causal FlashAttention-2 forward (mask key <= query, one sequence length), head dims 64 / 128: the sum-checked optimistic-softmax
// kernel of flash_attn_m16x.cuh (32 rows per wave, 256-row workgroups, 128-key tiles) with CAUSAL = true. Its own namespace, so the
// plain kernels' reachability table (fa2:: / fa:: in libcln_amd.so) is untouched; the product instantiations live in flash_attn_causal.hip.
// Why the sum-checked softmax holds under the mask: tile 0 adopts the true row maximum and every query row sees key 0 there, so the
// reference is finite from the first tile on; a masked score is -inf, adds exactly 0 to the row sum and never raises a maximum.
// One change (flash_attn_m16x_body.inc, cold path): only a row whose own check failed moves its reference, so no row's bits depend on
// the keys masked for it through another row of its wave.
#pragma once
#include "flash_attn_m16x.cuh"

namespace fa2c {
using namespace fa2;

template <int D_, int PD, int NDEF, int OX, int ORDER>
__global__ __launch_bounds__(512, 2) void fa2_fwd_m16x_causal_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K,
                                                                     const half_t* __restrict__ V, half_t* __restrict__ O,
                                                                     int N, int n_qblk, int n_heads, float scale_log2e) {
  constexpr int RPW_ = 32, BC_ = 128;
  constexpr bool VT = false, CAUSAL = true;
  constexpr bool LSE = false;
  [[maybe_unused]] unsigned long long* stamps = nullptr;
  [[maybe_unused]] float* lse = nullptr;
#include "flash_attn_m16x_body.inc"
}

template <int D_, int PD, int NDEF, int OX, int ORDER>
int launch_m16x_causal(const void* q, const void* k, const void* v, void* o, int B, int H, int N, hipStream_t stream) {
  using G = GeoM16<D_, 32, 128>;
  if (N % G::BR != 0) return CLN_ERR_UNSUPPORTED;
  static cln_lds_attr lds_attr;  // per device, thread-safe (common.h)
  if (cln_ensure_lds(lds_attr, reinterpret_cast<const void*>(&fa2_fwd_m16x_causal_kernel<D_, PD, NDEF, OX, ORDER>), G::LDS_BYTES) != CLN_OK) return CLN_ERR_LAUNCH;
  const float scale_log2e = 1.4426950408889634f / sqrtf((float)G::D);
  const int n_qblk = N / G::BR;
  CLN_LAUNCH((fa2_fwd_m16x_causal_kernel<D_, PD, NDEF, OX, ORDER>), dim3(n_qblk * B * H), dim3(G::NT), G::LDS_BYTES, stream,
             (const half_t*)q, (const half_t*)k, (const half_t*)v, (half_t*)o, N, n_qblk, B * H, scale_log2e);
  return cln_check_launch();
}

// the shipped options of the 32-rows-per-wave plain kernels (flash_attn_m16x.hip m16x_run): stages = 2 / stages = 1
constexpr int CAUSAL_OX = M16X_PRIO | M16X_SPLIT_PROLOGUE;
constexpr int CAUSAL_O1 = CAUSAL_OX | M16X_ONE_STAGE | (M16X_ONE_POS << M16X_ONE_POS_SHIFT);

template <int ORDER>
int run_causal(int D, bool one_stage, const void* q, const void* k, const void* v, void* o, int B, int H, int N, hipStream_t s) {
  if (D == 64) return one_stage ? launch_m16x_causal<64, 8, 4, CAUSAL_O1, ORDER>(q, k, v, o, B, H, N, s) : launch_m16x_causal<64, 8, 4, CAUSAL_OX, ORDER>(q, k, v, o, B, H, N, s);
  if (D == 128) return one_stage ? launch_m16x_causal<128, 4, 4, CAUSAL_O1, ORDER>(q, k, v, o, B, H, N, s) : launch_m16x_causal<128, 4, 4, CAUSAL_OX, ORDER>(q, k, v, o, B, H, N, s);
  return CLN_ERR_UNSUPPORTED;
}

}  // namespace fa2c
