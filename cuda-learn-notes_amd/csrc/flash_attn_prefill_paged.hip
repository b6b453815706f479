// Compile unit of the paged prefill attention entries cln_fa2_prefill_paged / cln_fa2_prefill_paged_describe (include/cln_amd_ext.h; kernel:
// flash_attn_prefill_paged.cuh).
#include "flash_attn_prefill_paged.cuh"

namespace {

// The checks that need no pointer: -1 for a non-positive dimension or Hq % Hkv != 0, -2 for another D, G or page, max_pages page >= 2^31, T G past
// an int or a grid that does not fit. *tiles = the row tiles (workgroups) per (sequence, KV head).
int prefill_shape(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, long long* tiles) {
  if (B <= 0 || T <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  const long long R = (long long)T * g->group;
  *tiles = (R + fa2pp::kRowTile - 1) / fa2pp::kRowTile;
  // the rows of a (sequence, KV head) are counted in an int; the workgroups, 256 threads each, all lie in x
  if (R > 0x7fffffffLL || *tiles > 0xffffffffLL / fa2pp::kThreads / B / Hkv) return CLN_ERR_UNSUPPORTED;
  return CLN_OK;
}

}  // namespace

CLN_API int cln_fa2_prefill_paged(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens, void* o,
                                  float* lse, int B, int T, int Hq, int Hkv, int P, int max_pages, int page, int D, void* stream) {
  const void* const in[] = {q, k_pages, v_pages, block_table, seqlens};  // 16-byte aligned up to the table, 4-byte from there on
  for (int i = 0; i < 5; ++i)
    if (!in[i] || !cln_aligned(in[i], i >= 3 ? 4 : 16)) return CLN_ERR_BAD_ARG;
  if (!o || !cln_aligned16(o) || !cln_aligned(lse, 4) || (const void*)lse == o) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 5; ++i)  // no output is an input
    if (o == in[i] || (lse && (const void*)lse == in[i])) return CLN_ERR_BAD_ARG;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  long long tiles = 0;
  const int rc = prefill_shape(B, T, Hq, Hkv, max_pages, page, D, &g, &tiles);
  if (rc != CLN_OK) return rc;
  const fa2d::PagedKV kv = {(const half_t*)k_pages, (const half_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  return D == 64 ? fa2pp::launch_prefill_paged<64>(q, kv, seqlens, o, lse, B, T, g.g_shift, tiles, s)
                 : fa2pp::launch_prefill_paged<128>(q, kv, seqlens, o, lse, B, T, g.g_shift, tiles, s);
}

CLN_API int cln_fa2_prefill_paged_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  long long tiles = 0;
  const int rc = prefill_shape(B, T, Hq, Hkv, max_pages, page, D, &g, &tiles);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len,
                         "fa2_prefill_paged<D=%d,G=%d> T=%d page=%d rows=%d keys=%d: one launch, no workspace; %lld workgroups of 256 threads (%lld "
                         "(sequence, KV head) pairs x %lld tiles of %d of the %lld query rows t G + g, 32 rows per wave), each walks the keys below "
                         "the causal edge of its last token in steps of %d, K and V rows through the block table to LDS once per workgroup, S^T = K "
                         "Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16, V through ds_read_b64_tr_b16, fp32 scores, causal mask by select on the "
                         "steps that cross the edge, online softmax, no split over the keys; deterministic",
                         D, g.group, T, page, fa2pp::kRowTile, fa2pp::kKeyStep, (long long)B * Hkv * tiles, (long long)B * Hkv, tiles,
                         fa2pp::kRowTile, (long long)T * g.group, fa2pp::kKeyStep);
  return n < len ? n : len - 1;
}
