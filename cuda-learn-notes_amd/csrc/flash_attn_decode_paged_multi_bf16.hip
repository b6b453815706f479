// Compile unit of the bf16 multi-token paged decode attention entries cln_fa2_decode_paged_multi_bf16_plan / cln_fa2_decode_paged_multi_bf16 /
// cln_fa2_decode_paged_multi_bf16_describe (include/cln_amd_ext.h; kernels: flash_attn_decode_paged_multi_bf16.cuh, paged_bf16.cuh). The plan,
// the checks and the status codes are those of flash_attn_decode_paged_multi.hip.
#include "flash_attn_decode_paged_multi_bf16.cuh"

namespace {

// The split plan of cln_fa2_decode_paged_multi_plan: the same function of the same seven numbers (the key step is the fp16 kernel's, the
// workspace is fp32 either way).
int multi_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  if (B <= 0 || T <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if ((D != 64 && D != 128) || T > fa2b::kMaxT) return CLN_ERR_UNSUPPORTED;
  return fa2d::split_plan((long long)B * Hkv, (long long)B * T * Hq, g->Nmax, page > fa2b::kMultiKeyStep ? page : fa2b::kMultiKeyStep, D, p);
}
int tiles_of(int T, const fa2d::PagedGeometry& g) { return (T * g.group + 15) / 16; }

template <int D>
int launch_tiles(int tiles, const void* q, const fa2b::PagedKV& kv, const int* sl, void* o, float* lse, void* ws, int B, int T, int gs, int S, int C,
                 hipStream_t s) {
  switch (tiles) {
    case 1: return fa2b::launch_decode_paged_multi<D, 1>(q, kv, sl, o, lse, ws, B, T, gs, S, C, s);
    case 2: return fa2b::launch_decode_paged_multi<D, 2>(q, kv, sl, o, lse, ws, B, T, gs, S, C, s);
    case 3: return fa2b::launch_decode_paged_multi<D, 3>(q, kv, sl, o, lse, ws, B, T, gs, S, C, s);
    default: return fa2b::launch_decode_paged_multi<D, 4>(q, kv, sl, o, lse, ws, B, T, gs, S, C, s);
  }
}

}  // namespace

CLN_API int cln_fa2_decode_paged_multi_bf16_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk,
                                                 long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode_paged_multi_bf16(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens,
                                            void* o, float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P,
                                            int max_pages, int page, int D, void* stream) {
  const void* in[] = {q, k_pages, v_pages, block_table, seqlens};
  int rc = fa2d::check_pointers(in, 5, 3, {o, lse, workspace});
  if (rc != CLN_OK) return rc;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  rc = multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p);
  if (rc != CLN_OK) return rc;
  if (!fa2d::workspace_fits(p, workspace, workspace_bytes)) return CLN_ERR_BAD_ARG;
  const fa2b::PagedKV kv = {(const bf16_t*)k_pages, (const bf16_t*)v_pages, block_table, Hkv, max_pages, g.page_shift};
  const hipStream_t s = (hipStream_t)stream;
  if (D == 64) return launch_tiles<64>(tiles_of(T, g), q, kv, seqlens, o, lse, workspace, B, T, g.g_shift, p.splits, p.chunk, s);
  return launch_tiles<128>(tiles_of(T, g), q, kv, seqlens, o, lse, workspace, B, T, g.g_shift, p.splits, p.chunk, s);
}

CLN_API int cln_fa2_decode_paged_multi_bf16_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = multi_plan(B, T, Hq, Hkv, max_pages, page, D, &g, &p);
  if (rc != CLN_OK) return rc;
  const int tiles = tiles_of(T, g);
  int n = snprintf(buf, len,
                   "fa2_decode_paged_multi_bf16_mfma<D=%d,MT=%d> T=%d G=%d S=%d C=%d page=%d: 4 waves split the %d-key steps, K rows through the block "
                   "table straight to MFMA fragments, V rows through a transposed LDS read, each row loaded once for the %d query rows (T x G, "
                   "%d tiles of 16) of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, fp32 scores, causal mask by "
                   "select, online softmax",
                   D, tiles, T, g.group, p.splits, p.chunk, page, fa2b::kMultiKeyStep, T * g.group, tiles);
  // fa2d::describe_tail with the name of the bf16-storing combine
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; then fa2_decode_combine_bf16_rows<D=%d> merges the live splits of a query row by log-sum-exp in ascending order (workspace %lld bytes)",
                  D, p.ws_bytes);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic");
  return n < len ? n : len - 1;
}
