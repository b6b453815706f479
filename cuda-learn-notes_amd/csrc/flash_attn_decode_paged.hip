// Compile unit of the paged decode attention entries cln_fa2_decode_paged_plan / cln_fa2_decode_paged / cln_fa2_decode_paged_describe
// (include/cln_amd_ext.h; kernels: flash_attn_decode_paged.cuh).
#include "flash_attn_decode_paged.cuh"
#include <stdio.h>
#include <string.h>

namespace {

// The split plan: a function of (B, Hq, Hkv, max_pages, page, D) only -- never of the lengths or the table, which stay on the device. A workgroup
// serves a whole group of query heads, so the workgroup count is B Hkv S. The constants are those of decode_plan (flash_attn_decode.hip):
constexpr int kTargetWorkgroups = 1024;  // split until B Hkv S reaches four workgroups per CU ...
constexpr int kMinChunk = 256;           // ... but give no workgroup fewer keys than this ...
constexpr int kMaxSplits = 64;           // ... and no head more partials than this

struct PagedPlan {
  int splits, chunk, group, page_shift;
  long long ws_bytes;
};

int paged_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, PagedPlan* p) {
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || max_pages <= 0 || page <= 0 || D <= 0 || Hq % Hkv != 0) return CLN_ERR_BAD_ARG;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return CLN_ERR_UNSUPPORTED;
  int shift = 0;
  while ((1 << shift) < page && shift < 9) ++shift;
  if ((1 << shift) != page || page < 16 || page > 256) return CLN_ERR_UNSUPPORTED;
  const long long Nmax = (long long)max_pages * page;
  if (Nmax > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  const long long step = fa2d::key_step(D), unit = page > step ? page : step, bk = (long long)B * Hkv;
  long long want = 1;
  if (bk < kTargetWorkgroups && Nmax > kMinChunk) {
    want = (kTargetWorkgroups + bk - 1) / bk;
    if (want > Nmax / kMinChunk) want = Nmax / kMinChunk;
    if (want > kMaxSplits) want = kMaxSplits;
  }
  const long long chunk = ((Nmax + want - 1) / want + unit - 1) / unit * unit;
  const long long splits = (Nmax + chunk - 1) / chunk;
  if (chunk > 0x7fffffffLL || (long long)B * Hq > 0x7fffffffLL || !fa2p::grid_fits(B, Hq, Hkv, (int)splits, D)) return CLN_ERR_UNSUPPORTED;
  p->splits = (int)splits, p->chunk = (int)chunk, p->group = G, p->page_shift = shift;
  p->ws_bytes = fa2p::workspace_bytes(B, Hq, p->splits, D);
  return CLN_OK;
}

template <int D>
int launch_group(int G, const void* q, const void* kp, const void* vp, const int* bt, const int* sl, void* o, float* lse, void* ws, int B, int Hkv,
                 int max_pages, const PagedPlan& p, hipStream_t s) {
  switch (G) {
    case 1: return fa2p::launch_decode_paged<D, 1>(q, kp, vp, bt, sl, o, lse, ws, B, Hkv, max_pages, p.page_shift, p.splits, p.chunk, s);
    case 2: return fa2p::launch_decode_paged<D, 2>(q, kp, vp, bt, sl, o, lse, ws, B, Hkv, max_pages, p.page_shift, p.splits, p.chunk, s);
    case 4: return fa2p::launch_decode_paged<D, 4>(q, kp, vp, bt, sl, o, lse, ws, B, Hkv, max_pages, p.page_shift, p.splits, p.chunk, s);
    default: return fa2p::launch_decode_paged<D, 8>(q, kp, vp, bt, sl, o, lse, ws, B, Hkv, max_pages, p.page_shift, p.splits, p.chunk, s);
  }
}

}  // namespace

CLN_API int cln_fa2_decode_paged_plan(int B, int Hq, int Hkv, int max_pages, int page, int D, int* splits, int* chunk, long long* workspace_bytes) {
  PagedPlan p;
  const int rc = paged_plan(B, Hq, Hkv, max_pages, page, D, &p);
  if (rc != CLN_OK) return rc;
  if (splits) *splits = p.splits;
  if (chunk) *chunk = p.chunk;
  if (workspace_bytes) *workspace_bytes = p.ws_bytes;
  return CLN_OK;
}

CLN_API int cln_fa2_decode_paged(const void* q, const void* k_pages, const void* v_pages, const int* block_table, const int* seqlens, void* o,
                                 float* lse, void* workspace, long long workspace_bytes, int B, int Hq, int Hkv, int P, int max_pages, int page, int D,
                                 void* stream) {
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
  PagedPlan p;
  const int rc = paged_plan(B, Hq, Hkv, max_pages, page, D, &p);
  if (rc != CLN_OK) return rc;
  if (p.splits > 1 && (!workspace || workspace_bytes < p.ws_bytes)) return CLN_ERR_BAD_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (D == 64) return launch_group<64>(p.group, q, k_pages, v_pages, block_table, seqlens, o, lse, workspace, B, Hkv, max_pages, p, s);
  return launch_group<128>(p.group, q, k_pages, v_pages, block_table, seqlens, o, lse, workspace, B, Hkv, max_pages, p, s);
}

CLN_API int cln_fa2_decode_paged_describe(int B, int Hq, int Hkv, int max_pages, int page, int D, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  PagedPlan p;
  const int rc = paged_plan(B, Hq, Hkv, max_pages, page, D, &p);
  if (rc != CLN_OK) return rc;
  int n = snprintf(buf, len,
                   "fa2_decode_paged<D=%d,G=%d> S=%d C=%d page=%d: 4 waves stream %d-key steps of K and V rows through the block table to registers, "
                   "each row loaded once for the %d query heads of its KV head, fp32 scores, online softmax",
                   D, p.group, p.splits, p.chunk, page, fa2d::key_step(D), p.group);
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n,
                  "; then fa2_decode_paged_combine<D=%d> merges the live splits of a query head by log-sum-exp in ascending order (workspace %lld bytes)",
                  D, p.ws_bytes);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic");
  return n < len ? n : len - 1;
}
