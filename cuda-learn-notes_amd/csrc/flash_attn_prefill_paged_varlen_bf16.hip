// Compile unit of the bf16 packed variable-length paged prefill attention entries cln_fa2_prefill_paged_varlen_bf16 /
// cln_fa2_prefill_paged_varlen_bf16_describe (include/cln_amd_ext.h; kernel: flash_attn_prefill_paged_varlen_bf16.cuh). The checks and the
// status codes are those of flash_attn_prefill_paged_varlen.hip.
#include "flash_attn_prefill_paged_varlen_bf16.cuh"

namespace {

// The checks that need no pointer: -1 for a non-positive dimension or Hq % Hkv != 0, -2 for another D, G or page, max_pages page >= 2^31 or a grid
// that does not fit. *slots = the workgroups per KV head, a function of B, total_q and G alone: the offsets stay on the device.
int varlen_shape(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, long long* slots) {
  if (B <= 0 || total_q <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  const long long R = (long long)total_q * g->group;
  *slots = R / fa2b::kRowTile + B;
  // the packed rows times G are counted in an int; the workgroups, 256 threads each, all lie in x
  if (R > 0x7fffffffLL || *slots > 0xffffffffLL / fa2b::kThreads / Hkv) return CLN_ERR_UNSUPPORTED;
  return CLN_OK;
}

}  // namespace

CLN_API int cln_fa2_prefill_paged_varlen_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                              const int* cu_q, void* o, float* lse, int B, int total_q, int Hq, int Hkv, int P, int max_pages,
                                              int page, int D, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens, cu_q};  // 16-byte aligned up to the table, 4-byte from there on
  for (int i = 0; i < 6; ++i)
    if (!in[i] || !cln_aligned(in[i], i >= 3 ? 4 : 16)) return CLN_ERR_BAD_ARG;
  if (!o || !cln_aligned16(o) || !cln_aligned(lse, 4) || (const void*)lse == o) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 6; ++i)  // no output is an input
    if (o == in[i] || (lse && (const void*)lse == in[i])) return CLN_ERR_BAD_ARG;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  long long slots = 0;
  const int rc = varlen_shape(B, total_q, Hq, Hkv, max_pages, page, D, &g, &slots);
  if (rc != CLN_OK) return rc;
  const fa2b::PagedKV kv = {(const bf16_t*)k_pages, (const bf16_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return D == 64 ? fa2b::launch_prefill_paged_varlen<64>(q, kv, seqlens, cu_q, o, lse, B, total_q, g.g_shift, slots, s)
                 : fa2b::launch_prefill_paged_varlen<128>(q, kv, seqlens, cu_q, o, lse, B, total_q, g.g_shift, slots, s);
}

CLN_API int cln_fa2_prefill_paged_varlen_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  long long slots = 0;
  const int rc = varlen_shape(B, total_q, Hq, Hkv, max_pages, page, D, &g, &slots);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "fa2_prefill_paged_varlen_bf16_mfma<D=%d,G=%d> B=%d total_q=%d page=%d rows=%d keys=%d: one launch, no workspace; %lld "
                         "workgroups of 256 threads (%d KV heads x %lld slots = total_q G / %d + B, at most B of them empty), sequence b owns the "
                         "slots from cu_q[b] G / %d + b, found by binary search over the device-side offsets; a slot is a tile of %d of the T_b G "
                         "query rows t G + g of its sequence, 32 rows per wave, and walks the keys below the causal edge of its last token in "
                         "steps of %d, K and V rows through the block table to LDS once per workgroup, S^T = K Q^T and O^T = V^T P^T on "
                         "v_mfma_f32_16x16x32_bf16, V through ds_read_b64_tr_b16, fp32 scores, causal mask by select on the steps that cross the "
                         "edge, online softmax, no split over the keys; deterministic",
                         D, g.group, B, total_q, page, fa2b::kRowTile, fa2b::kKeyStep, (long long)Hkv * slots, Hkv, slots, fa2b::kRowTile,
                         fa2b::kRowTile, fa2b::kRowTile, fa2b::kKeyStep);
  return n < len ? n : len - 1;
}
