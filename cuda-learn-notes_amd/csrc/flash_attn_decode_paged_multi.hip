// Compile unit of the multi-token paged decode attention entries cln_fa2_decode_paged_multi_plan / cln_fa2_decode_paged_multi /
// cln_fa2_decode_paged_multi_describe (include/cln_amd_ext.h; kernels: flash_attn_decode_paged_multi.cuh).
#include "flash_attn_decode_paged_multi.cuh"
#include <stdio.h>
#include <string.h>

namespace {

// The split plan: a function of (B, T, Hq, Hkv, max_pages, page, D) only -- never of the lengths or the table, which stay on the device. It is the
// plan of cln_fa2_decode_paged (flash_attn_decode_paged.hip) with the key step of this kernel: a workgroup serves all T G query rows
// of a (sequence, KV head, split), so the workgroup count is B Hkv S whatever T is.
constexpr int kTargetWorkgroups = 1024;  // split until B Hkv S reaches four workgroups per CU ...
constexpr int kMinChunk = 256;           // ... but give no workgroup fewer keys than this ...
constexpr int kMaxSplits = 64;           // ... and no query row more partials than this

struct MultiPlan {
  int splits, chunk, group, g_shift, page_shift, tiles;
  long long ws_bytes;
};

int multi_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, MultiPlan* p) {
  if (B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || max_pages <= 0 || page <= 0 || D <= 0 || Hq % Hkv != 0) return CLN_ERR_BAD_ARG;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  if (T > fa2pm::kMaxT) return CLN_ERR_UNSUPPORTED;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return CLN_ERR_UNSUPPORTED;
  int shift = 0;
  while ((1 << shift) < page && shift < 9) ++shift;
  if ((1 << shift) != page || page < 16 || page > 256) return CLN_ERR_UNSUPPORTED;
  const long long Nmax = (long long)max_pages * page;
  if (Nmax > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  const long long step = fa2pm::kKeyStep, unit = page > step ? page : step, bk = (long long)B * Hkv;
  long long want = 1;
  if (bk < kTargetWorkgroups && Nmax > kMinChunk) {
    want = (kTargetWorkgroups + bk - 1) / bk;
    if (want > Nmax / kMinChunk) want = Nmax / kMinChunk;
    if (want > kMaxSplits) want = kMaxSplits;
  }
  const long long chunk = ((Nmax + want - 1) / want + unit - 1) / unit * unit;
  const long long splits = (Nmax + chunk - 1) / chunk;
  if (chunk > 0x7fffffffLL || (long long)B * T * Hq > 0x7fffffffLL || !fa2pm::grid_fits(B, T, Hq, Hkv, (int)splits, D)) return CLN_ERR_UNSUPPORTED;
  p->splits = (int)splits, p->chunk = (int)chunk, p->group = G, p->page_shift = shift;
  p->g_shift = G == 1 ? 0 : G == 2 ? 1 : G == 4 ? 2 : 3;
  p->tiles = (T * G + 15) / 16;
  p->ws_bytes = fa2pm::workspace_bytes(B, T, Hq, p->splits, D);
  return CLN_OK;
}

template <int D>
int launch_tiles(const void* q, const void* kp, const void* vp, const int* bt, const int* sl, void* o, float* lse, void* ws, int B, int T, int Hkv,
                 int max_pages, const MultiPlan& p, hipStream_t s) {
  const int gs = p.g_shift, ps = p.page_shift, S = p.splits, C = p.chunk;
  switch (p.tiles) {
    case 1: return fa2pm::launch_decode_paged_multi<D, 1>(q, kp, vp, bt, sl, o, lse, ws, B, T, Hkv, gs, max_pages, ps, S, C, s);
    case 2: return fa2pm::launch_decode_paged_multi<D, 2>(q, kp, vp, bt, sl, o, lse, ws, B, T, Hkv, gs, max_pages, ps, S, C, s);
    case 3: return fa2pm::launch_decode_paged_multi<D, 3>(q, kp, vp, bt, sl, o, lse, ws, B, T, Hkv, gs, max_pages, ps, S, C, s);
    default: return fa2pm::launch_decode_paged_multi<D, 4>(q, kp, vp, bt, sl, o, lse, ws, B, T, Hkv, gs, max_pages, ps, S, C, s);
  }
}

}  // namespace

CLN_API int cln_fa2_decode_paged_multi_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk,
                                            long long* workspace_bytes) {
  MultiPlan p;
  const int rc = multi_plan(B, T, Hq, Hkv, max_pages, page, D, &p);
  if (rc != CLN_OK) return rc;
  if (splits) *splits = p.splits;
  if (chunk) *chunk = p.chunk;
  if (workspace_bytes) *workspace_bytes = p.ws_bytes;
  return CLN_OK;
}

CLN_API int cln_fa2_decode_paged_multi(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens, void* o,
                                       float* lse, void* workspace, long long workspace_bytes, int B, int T, int Hq, int Hkv, int P, int max_pages,
                                       int page, int D, void* stream) {
  const void* in[] = {q, k_pages, v_pages, block_table, seqlens};
  const void* out[] = {o, lse, workspace};  // lse and workspace may be null
  for (int i = 0; i < 5; ++i)
    if (!in[i] || !cln_aligned(in[i], i >= 3 ? 4 : 16)) return CLN_ERR_BAD_ARG;
  if (!o) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 3; ++i) {
    if (!out[i]) continue;
    if (!cln_aligned16(out[i])) return CLN_ERR_BAD_ARG;
    for (const void* p : in)
      if (out[i] == p) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < i; ++j)
      if (out[i] == out[j]) return CLN_ERR_BAD_ARG;
  }
  if (P <= 0) return CLN_ERR_BAD_ARG;
  MultiPlan p;
  const int rc = multi_plan(B, T, Hq, Hkv, max_pages, page, D, &p);
  if (rc != CLN_OK) return rc;
  if (p.splits > 1 && (!workspace || workspace_bytes < p.ws_bytes)) return CLN_ERR_BAD_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (D == 64) return launch_tiles<64>(q, k_pages, v_pages, block_table, seqlens, o, lse, workspace, B, T, Hkv, max_pages, p, s);
  return launch_tiles<128>(q, k_pages, v_pages, block_table, seqlens, o, lse, workspace, B, T, Hkv, max_pages, p, s);
}

CLN_API int cln_fa2_decode_paged_multi_describe(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  MultiPlan p;
  const int rc = multi_plan(B, T, Hq, Hkv, max_pages, page, D, &p);
  if (rc != CLN_OK) return rc;
  int n = snprintf(buf, len,
                   "fa2_decode_paged_multi<D=%d,MT=%d> T=%d G=%d S=%d C=%d page=%d: 4 waves split the %d-key steps, K rows through the block table "
                   "straight to MFMA fragments, V rows through a transposed LDS read, each row loaded once for the %d query rows (T x G, %d tiles of "
                   "16) of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16, fp32 scores, causal mask by select, online softmax",
                   D, p.tiles, T, p.group, p.splits, p.chunk, page, fa2pm::kKeyStep, T * p.group, p.tiles);
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; then fa2_decode_paged_multi_combine<D=%d> merges the live splits of a query row by log-sum-exp in ascending order (workspace "
                  "%lld bytes)",
                  D, p.ws_bytes);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic");
  return n < len ? n : len - 1;
}
