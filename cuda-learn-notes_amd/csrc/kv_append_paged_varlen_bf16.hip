// Compile unit of the bf16 packed variable-length paged KV-cache append entries cln_kv_append_paged_varlen_bf16 /
// cln_kv_append_paged_varlen_bf16_describe (include/cln_amd_ext.h; kernel: kv_append_paged_varlen_bf16.cuh). The checks and the status codes are
// those of kv_append_paged_varlen.hip.
#include "kv_append_paged_varlen_bf16.cuh"

namespace {

// The checks that need no pointer: -1 for a non-positive dimension or Hq % Hkv != 0, -2 for another D, page or rope_mode, max_pages page >= 2^31
// or a grid that does not fit. *y = the workgroups per packed row.
int append_shape(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode, bool has_q, int* page_shift, long long* y) {
  if (B <= 0 || total_q <= 0 || D <= 0 || Hq <= 0 || Hkv <= 0 || max_pages <= 0 || page <= 0 || Hq % Hkv != 0) return CLN_ERR_BAD_ARG;
  if ((D != 64 && D != 128) || rope_mode < 0 || rope_mode > 2) return CLN_ERR_UNSUPPORTED;
  fa2d::PagedGeometry g;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, &g);  // the page size and max_pages page; the group size is of no concern here
  if (rc != CLN_OK) return rc;
  *page_shift = g.page_shift;
  *y = kva::grid_y(1, total_q, Hq, Hkv, has_q, D, rope_mode);
  return *y > 0 ? CLN_OK : CLN_ERR_UNSUPPORTED;
}

template <int D>
int launch_mode(int rope_mode, const kva::ArgsVarlenBf16& a, long long y, hipStream_t s) {
  switch (rope_mode) {
    case 0: return kva::launch_varlen_bf16<D, 0>(a, y, s);
    case 1: return kva::launch_varlen_bf16<D, 1>(a, y, s);
    default: return kva::launch_varlen_bf16<D, 2>(a, y, s);
  }
}

}  // namespace

CLN_API int cln_kv_append_paged_varlen_bf16(const void* k_new, const void* v_new, void* k_pages, void* v_pages, const int* block_table,
                                            const int* seqlens, const int* cu_q, const void* q, void* q_out, const float* rope_table, int B,
                                            int total_q, int Hq, int Hkv, int P, int max_pages, int page, int D, int max_pos, int rope_mode,
                                            void* stream) {
  const void* const in[] = {k_new, v_new, block_table, seqlens, cu_q, q, rope_table};  // 16-byte aligned up to first4, 4-byte from there on ...
  const int first4[] = {0, 0, 1, 1, 1, 0, 1};
  const void* const out[] = {k_pages, v_pages, q_out};
  for (int i = 0; i < 5; ++i)
    if (!in[i]) return CLN_ERR_BAD_ARG;
  if (!k_pages || !v_pages) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 7; ++i)
    if (in[i] && !cln_aligned(in[i], first4[i] ? 4 : 16)) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 3; ++i) {  // ... and no output is another output or an input, but q_out may be q: a thread reads its pairs before it writes
    if (!out[i]) continue;
    if (!cln_aligned16(out[i])) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < i; ++j)
      if (out[i] == out[j]) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < 7; ++j)
      if (out[i] == in[j] && !(i == 2 && j == 5)) return CLN_ERR_BAD_ARG;
  }
  if (P <= 0) return CLN_ERR_BAD_ARG;
  if (rope_mode == 0 && (q || q_out || rope_table)) return CLN_ERR_BAD_ARG;
  if ((rope_mode == 1 || rope_mode == 2) && (!rope_table || max_pos <= 0 || (q == nullptr) != (q_out == nullptr))) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = append_shape(B, total_q, Hq, Hkv, max_pages, page, D, rope_mode, q != nullptr, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  const kva::ArgsVarlenBf16 a = {(const bf16_t*)k_new, (const bf16_t*)v_new, (bf16_t*)k_pages, (bf16_t*)v_pages, block_table, seqlens, cu_q,
                                 (const bf16_t*)q, (bf16_t*)q_out, rope_table, B, total_q, Hq, Hkv, P, max_pages, page_shift, max_pos};
  const hipStream_t s = (hipStream_t)stream;
  return D == 64 ? launch_mode<64>(rope_mode, a, y, s) : launch_mode<128>(rope_mode, a, y, s);
}

CLN_API int cln_kv_append_paged_varlen_bf16_describe(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode, char* buf,
                                                     int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  int page_shift = 0;
  long long y = 0;
  const int rc = append_shape(B, total_q, Hq, Hkv, max_pages, page, D, rope_mode, rope_mode != 0, &page_shift, &y);
  if (rc != CLN_OK) return rc;
  static const char* const kRot[] = {"rows copied bit for bit", "K and q rotated in half-split pairs (i, i + D/2)", "K and q rotated in interleaved pairs (2i, 2i + 1)"};
  const int n = snprintf(buf, len,
                         "kv_append_paged_varlen_bf16_rows<D=%d,ROPE=%d> B=%d total_q=%d page=%d: one launch, no workspace; %d x %lld workgroups of 256 "
                         "threads (a packed row x the 16-byte pieces of its %d K, %d V and %d q rows), the sequence of a row by binary search over "
                         "the device-side offsets, length and table entry through uniform loads, %s%s, plain stores into the pools; deterministic",
                         D, rope_mode, B, total_q, page, total_q, y, Hkv, Hkv, rope_mode ? Hq : 0, kRot[rope_mode],
                         rope_mode ? " in fp32 from the cos/sin table with one rounding at the store, V copied" : "");
  return n < len ? n : len - 1;
}
