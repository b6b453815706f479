// FlashAttention-2 forward, head dims 64 / 128: the 16x16x32 ping-pong kernel of flash_attn_m16.cuh with a SUM-CHECKED
// OPTIMISTIC softmax (round 3). Reference rung: kernels/flash-attn/mma/basic/flash_attn_mma_share_qkv.cu:66.
//
// What changes against flash_attn_m16.cuh, and why. That kernel computes, per KV tile, the row maximum of all scores
// (a serial v_max3 chain + two cross-lane swaps, ~40 of its ~190 VALU instructions per wave and tile), decides whether
// the running reference m must move, and only then starts the exponentials: inside a wave the QK^T MFMAs, the maximum
// and the exponentials are strictly serial. But the maximum is only ever USED to keep P = 2^(s - m) inside fp16
// (the reference m is deferred anyway: it moves only when a row grew by more than 2^8). So:
//   * the S^T accumulators start at -m (as before) and every 16-key block is exponentiated AS SOON AS its MFMA chain
//     has finished, relative to the current reference, while the MFMAs of the next key block run -- no maximum first;
//   * the row sums that the softmax needs anyway are the overflow check: if the per-lane partial sum of a tile is
//     <= 2^15, every P of it is <= 2^15 and fits fp16; inf / NaN fail the comparison too. One compare per query block
//     and tile replaces the max chain;
//   * only when a lane fails the check (or on tile 0, which has no reference yet) the wave takes the COLD path: the true
//     row maxima of the tile, the standard rescale of O / l / the pending scores, and the exponentials again.
//   * the exponentials of the last NDEF key blocks are issued in phase B under the PV MFMAs (their scores are checked
//     directly against 14 at the end of phase A: 4 v_max3 per block instead of a sum that does not exist yet).
// fp16 has the same relative precision from 2^-14 to 2^15 and O / l accumulate in fp32, so a reference that lags the true
// maximum by up to 15 binades costs nothing (the deferred form already allowed 8); the reference never moves down, and
// tile 0 adopts its true maximum, so the largest P of a row is always >= 1.
// Phase A (QK^T + exponentials) is now VALU-dense and phase B (PV) MFMA-only: with OX & 1 the wave raises its priority
// in phase A so its VALU instructions win the issue arbitration against the partner's MFMAs (the matrix pipe needs one
// issue slot per 16 cycles).
#pragma once
#include "flash_attn_m16.cuh"

namespace fa2 {

// OX bits. Production uses M16X_PRIO | M16X_SPLIT_PROLOGUE (= 5); everything from M16X_PRIO_STATIC up is instantiated only in the
// probe library (probe/flash_attn_m16x_probe.hip) and its measured effect is in profiles/r03_fa_c4_ablation_probe.log.
enum : int {
  M16X_PRIO = 1,            // s_setprio 1 in phase A (VALU-dense), 0 in phase B
  M16X_PRIO_B = 2,          // the opposite flip
  M16X_SPLIT_PROLOGUE = 4,  // tile 0's DMA pieces before the Q loads; group 1 does not hold up the first barrier
  M16X_PRIO_STATIC = 8,     // s_setprio 1 once for the group that runs a phase behind, no flips
  M16X_NT_STORE = 16,       // non-temporal O stores
  // ablations (results are garbage by design): no K fragment reads, no V fragment reads, no exponentials, no LDS-DMA after the
  // prologue, no workgroup barriers inside the KV loop (the last only together with the LDS ablations)
  M16X_ABL_K = 32, M16X_ABL_V = 64, M16X_ABL_EXP = 128, M16X_ABL_DMA = 256, M16X_ABL_BAR = 1024,
  // QK^T steps of TWO key blocks interleaved (kb, kb+1 at k-step 0, then both at k-step 1): a dependent MFMA on one accumulator
  // then sits 2 * NQB MFMAs behind the one it depends on instead of NQB (D = 64: NKS = 2)
  M16X_PAIRED_QK = 512,
  M16X_SNAKE = 2048,  // query blocks in snake order (0,1 | 1,0 | ...): every MFMA shares one operand register set with its predecessor
  M16X_FINE = 4096,   // one softmax item behind EACH MFMA (M V M V) instead of the step's MFMAs first and its items after them
  // phase A exponentiates its NOPT blocks behind the LAST NOPT blocks' MFMAs instead of the first ones: a wave's softmax-carrying stretch is
  // then [second half of A, first half of B] and its bare-MFMA stretch [second half of B, first half of A]; the partner group runs one phase
  // behind, so one wave of a SIMD is always in its bare stretch while the other carries softmax work. With M16X_PRIO the priority follows
  // the stretches (1 while carrying softmax work) instead of the phases.
  M16X_LATE = 8192,
  // the deferred key blocks are not checked by their raw scores at the end of phase A (NDEF * NQB * 4 scores through v_max3 per lane and
  // tile); instead their OWN partial row sums are compared once, in phase B, right after their last exponential and before the first PV
  // MFMA that consumes them -- a failing wave rescales O / l there (the PV products of the optimistic blocks are already in O, relative
  // to the old reference, and are scaled with it) and exponentiates the deferred blocks again
  M16X_LATE_CHECK = 16384,
  // the `stages = 1` form (reference kStage = 1, flash_attn_mma_share_qkv.cu:711-762: a tile is requested, waited for, then used): the
  // SAME kernel, same LDS image and arithmetic (bit-identical output), but a wave issues all its pieces of tile j + 1 in ONE burst and
  // waits for them right there (s_waitcnt vmcnt(0)): no request of the wave is in flight while it computes. M16X_ONE_POS (probe) picks the
  // burst's place in the iteration: 0 = top of phase A, 1 = end of phase A, 2 = top of phase B, 3 = end of phase B.
  M16X_ONE_STAGE = 32768,
  M16X_ONE_POS_SHIFT = 16,  // two bits
  // scores scaled in fp32 (round 4; the reference's *_acc_f32 names): Q goes into the MFMAs as loaded, S^T accumulates from 0 and every score takes
  // one v_fma_f32 (s * log2(e)/sqrt(d) - m) on its way into v_exp_f32 -- no fp16 rounding of Q * log2(e)/sqrt(d) (2^-11 relative per term, which
  // amplified keys turn into 3.9e-3 on O where this form has 2e-3), 64 more VALU instructions per wave and 128-key tile at D = 64
  M16X_FSCALE = 1 << 18,
  // probe (round 4; the "one untested trade" of DESIGN_LOG 9.3): ROW SUMS ON THE MATRIX PIPE. l = sum of the fp16 P values, from one more MFMA per
  // 32-key step and query block with an all-ones A operand (every row of its 16x16 result is the row-sum vector, so no cross-lane reduction at the
  // end either); the 64 v_add_f32 per tile go, and the fp16-overflow check of the optimistic blocks becomes a running v_max3 of the exponents (<= 15).
  M16X_MFMA_SUM = 1 << 19,
  // probe (round 5): the partial row sums by v_dot2_f32_f16 -- acc += p0 + p1 over the fp16-ROUNDED pair in ONE instruction instead of two v_add_f32 (64 -> 32
  // row-sum instructions per wave and 128-key tile at D = 64); l becomes the sum of the same fp16 values the numerator uses, an fp16 overflow still fails the check (inf)
  M16X_DOT2_SUM = 1 << 20,
  // probe (round 6, VERDICT r5 #1b "C4's fixed cost"): every wave stamps s_memrealtime (100 MHz, chip-wide) and s_memtime (shader clock) at kernel entry,
  // at the top of the KV loop (prologue done), behind the loop and behind its last O store (waited for), plus its HW_ID / XCC_ID -- 10 words per wave into
  // g_m16x_stamps (probe library: cln_probe_set_stamps). tools/fa_c4_stamps.py turns them into the launch ramp, prologue, per-tile and tail times per CU.
  M16X_STAMP = 1 << 21,
  M16X_ONE_POS = 2           // the shipped position: top of phase B (the MFMA-only phase), 0.95-1.0x of stages = 2 (profiles/r04_fa_one_stage_probe.log)
};

// Launch orders of the causal kernel (flash_attn_causal.cuh; CAUSAL = true only). Row block qb of a head runs 2 (qb + 1) key tiles.
enum : int {
  M16X_ORDER_PLAIN = 0,    // the plain kernel's mapping: heads pinned to XCDs, the row blocks of a head in ascending order
  M16X_ORDER_HEAVY = 1,    // heads pinned to XCDs, each XCD walks the row blocks of ALL its heads heaviest first (the last qb of every head, then the one before)
  M16X_ORDER_HEAD_REV = 2  // the plain mapping with the row blocks of each head in descending order
};

inline unsigned long long* g_m16x_stamps = nullptr;  // device buffer of the M16X_STAMP probe form (10 words per wave); never set in the product library

template <int D_, int RPW_, int BC_, int PD = 4, int NDEF = 1, int OX = 0, bool VT = false>
__global__ __launch_bounds__(512, 2) void fa2_fwd_m16x_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K,
                                                              const half_t* __restrict__ V, half_t* __restrict__ O,
                                                              int N, int n_qblk, int n_heads, float scale_log2e, unsigned long long* stamps) {
  constexpr bool CAUSAL = false;
  constexpr int ORDER = M16X_ORDER_PLAIN;
  constexpr bool LSE = false;
  [[maybe_unused]] float* lse = nullptr;
#include "flash_attn_m16x_body.inc"
}

template <int D_, int RPW_, int BC_, int PD = 4, int NDEF = 1, int OX = 0, bool VT = false>
int launch_m16x(const void* q, const void* k, const void* v, void* o, int B, int H, int N, hipStream_t stream) {
  using G = GeoM16<D_, RPW_, BC_>;
  if (N % G::BR != 0) return CLN_ERR_UNSUPPORTED;
  static cln_lds_attr lds_attr;  // per device, thread-safe (common.h)
  if (cln_ensure_lds(lds_attr, reinterpret_cast<const void*>(&fa2_fwd_m16x_kernel<D_, RPW_, BC_, PD, NDEF, OX, VT>), G::LDS_BYTES) != CLN_OK) return CLN_ERR_LAUNCH;
  const float scale_log2e = 1.4426950408889634f / sqrtf((float)G::D);
  const int n_qblk = N / G::BR;
  CLN_LAUNCH((fa2_fwd_m16x_kernel<D_, RPW_, BC_, PD, NDEF, OX, VT>), dim3(n_qblk * B * H), dim3(G::NT), G::LDS_BYTES, stream,
             (const half_t*)q, (const half_t*)k, (const half_t*)v, (half_t*)o, N, n_qblk, B * H, scale_log2e, (OX & M16X_STAMP) != 0 ? g_m16x_stamps : nullptr);
  return cln_check_launch();
}

}  // namespace fa2
