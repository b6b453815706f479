// Compile unit of the bf16 multi-head latent attention (MLA) prefill for a packed batch: cln_fa2_prefill_varlen_mla_bf16 /
// cln_fa2_prefill_varlen_mla_bf16_describe (include/cln_amd_ext.h; kernel: flash_attn_prefill_varlen_mla_bf16.cuh). The checking
// order and the status codes are the siblings': the scale first (required, finite, > 0: -1, paged::mla_scale_arg), then the pointers (-1), then
// the shape (paged::mla_prefill_shape: -1 for a non-positive dimension, -2 for Hq > 128, another causal flag or a grid that does not fit).
#include "flash_attn_prefill_varlen_mla_bf16.cuh"
#include "paged_entry.h"

static_assert(fa2mp::kDn == paged::kMlaDn && fa2mp::kDr == paged::kMlaDr && fa2mp::kDk == paged::kMlaDq && fa2mp::kDv == paged::kMlaDv,
              "paged::mla_prefill_shape and the describe text speak of this kernel's dims");

CLN_API int cln_fa2_prefill_varlen_mla_bf16(const void* q, const void* kv, const void* k_pe, const int* cu_q, const int* cu_k, void* o, float* lse,
                                            int B, int total_q, int total_k, int Hq, int causal, float softmax_scale, void* stream) {
  float mult = 0.0f;
  int rc = paged::mla_scale_arg(softmax_scale, &mult);
  if (rc != CLN_OK) return rc;
  rc = paged::mla_prefill_args(q, kv, k_pe, cu_q, cu_k, o, lse);
  if (rc != CLN_OK) return rc;
  long long slots = 0;
  rc = paged::mla_prefill_shape(B, total_q, total_k, Hq, causal, &slots);
  if (rc != CLN_OK) return rc;
  const fa2mp::Args a = {(const bf16_t*)q, (const bf16_t*)kv, (const bf16_t*)k_pe, cu_q, cu_k, (bf16_t*)o, lse, B, total_q, total_k, Hq, causal,
                         (unsigned)slots, mult};
  return fa2mp::launch_prefill_varlen_mla(a, (hipStream_t)stream);
}

CLN_API int cln_fa2_prefill_varlen_mla_bf16_describe(int B, int total_q, int total_k, int Hq, int causal, float softmax_scale, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  float mult = 0.0f;
  int rc = paged::mla_scale_arg(softmax_scale, &mult);
  if (rc != CLN_OK) return rc;
  long long slots = 0;
  rc = paged::mla_prefill_shape(B, total_q, total_k, Hq, causal, &slots);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "fa2_prefill_varlen_mla_bf16_mfma<Dk=%d,Dv=%d> softmax_scale=%.9g (the caller's), score multiplier x log2(e) = %.9g; B=%d "
                         "total_q=%d total_k=%d Hq=%d %s: one launch, no workspace; %lld slots per head (total_q / %d + B), grid %lld workgroups of 4 "
                         "waves, a 128-row tile of one (sequence, head) each, 32 rows per wave, the sequence of a slot by binary search over the "
                         "device-side offsets; per %d-key step the workgroup stages k_nope (%d dims) and v (%d dims) of its head from kv rows of %d and "
                         "the one k_pe row (%d dims) every head shares into LDS (%d bytes static: K rows of %d bytes, V rows of %d), the next step's "
                         "rows waiting in registers; %d MFMAs per wave and step on v_mfma_f32_16x16x32_bf16: S^T = K Q^T over 6 k-steps of 32 dims (4 "
                         "k_nope + 2 k_pe, 48) and O^T = V^T P^T through transposing reads (32), fp32 scores and accumulators, %s, online softmax, P "
                         "and O rounded once to bf16, a query that sees no key O = 0, LSE = -inf; deterministic",
                         paged::kMlaDq, paged::kMlaDv, (double)softmax_scale, (double)mult, B, total_q, total_k, Hq, causal ? "causal" : "non-causal",
                         slots, fa2pp::kRowTile, (long long)Hq * slots, fa2pp::kKeyStep, paged::kMlaDn, paged::kMlaDv, fa2mp::kKvRow, paged::kMlaDr,
                         fa2mp::kLdsBytes, fa2mp::kKRowB, fa2mp::kVRowB, fa2mp::kMfmasPerStep,
                         causal ? "query t of a sequence sees the keys j < L - (T - 1 - t), masked by select" : "every query sees all L keys of its sequence");
  return n < len ? n : len - 1;
}
