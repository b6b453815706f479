// Compile unit of the decode attention entries cln_fa2_decode_plan / cln_fa2_decode (include/cln_amd_ext.h; kernels: flash_attn_decode.cuh).
#include "flash_attn_decode.cuh"
#include <stdio.h>
#include <string.h>

namespace {

// The split plan: a function of (B, H, Nmax, D) only -- never of the lengths, which stay on the device -- so the bits of a sequence do not depend
// on its neighbours. The constants come from the sweep of tools/fa_decode_probe.py:
constexpr int kTargetWorkgroups = 1024;  // split until B H S reaches four workgroups per CU ...
constexpr int kMinChunk = 256;           // ... but give no workgroup fewer keys than this ...
constexpr int kMaxSplits = 64;           // ... and no head more partials than this

struct DecodePlan {
  int splits, chunk;
  long long ws_bytes;
};

int decode_plan(int B, int H, int Nmax, int D, DecodePlan* p) {
  if (B <= 0 || H <= 0 || Nmax <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  const long long step = fa2d::key_step(D), bh = (long long)B * H;
  long long want = 1;
  if (bh < kTargetWorkgroups && Nmax > kMinChunk) {
    want = (kTargetWorkgroups + bh - 1) / bh;
    if (want > Nmax / kMinChunk) want = Nmax / kMinChunk;
    if (want > kMaxSplits) want = kMaxSplits;
  }
  const long long chunk = ((Nmax + want - 1) / want + step - 1) / step * step;
  const long long splits = (Nmax + chunk - 1) / chunk;
  if (chunk > 0x7fffffffLL || bh > 0x7fffffffLL || !fa2d::grid_fits(B, H, (int)splits)) return CLN_ERR_UNSUPPORTED;
  p->splits = (int)splits, p->chunk = (int)chunk;
  p->ws_bytes = fa2d::workspace_bytes(B, H, p->splits, D);
  return CLN_OK;
}

}  // namespace

CLN_API int cln_fa2_decode_plan(int B, int H, int Nmax, int D, int* splits, int* chunk, long long* workspace_bytes) {
  DecodePlan p;
  const int rc = decode_plan(B, H, Nmax, D, &p);
  if (rc != CLN_OK) return rc;
  if (splits) *splits = p.splits;
  if (chunk) *chunk = p.chunk;
  if (workspace_bytes) *workspace_bytes = p.ws_bytes;
  return CLN_OK;
}

CLN_API int cln_fa2_decode(const void* q, const void* k_cache, const void* v_cache, const int* seqlens, void* o, float* lse, void* workspace,
                           long long workspace_bytes, int B, int H, int Nmax, int D, void* stream) {
  const void* in[] = {q, k_cache, v_cache, seqlens};
  const void* out[] = {o, lse, workspace};  // lse and workspace may be null
  for (int i = 0; i < 4; ++i)
    if (!in[i] || !cln_aligned(in[i], i == 3 ? 4 : 16)) return CLN_ERR_BAD_ARG;
  if (!o) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 3; ++i) {
    if (!out[i]) continue;
    if (!cln_aligned16(out[i])) return CLN_ERR_BAD_ARG;
    for (const void* p : in)
      if (out[i] == p) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < i; ++j)
      if (out[i] == out[j]) return CLN_ERR_BAD_ARG;
  }
  DecodePlan p;
  const int rc = decode_plan(B, H, Nmax, D, &p);
  if (rc != CLN_OK) return rc;
  if (p.splits > 1 && (!workspace || workspace_bytes < p.ws_bytes)) return CLN_ERR_BAD_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (D == 64) return fa2d::launch_decode<64>(q, k_cache, v_cache, seqlens, o, lse, workspace, B, H, Nmax, p.splits, p.chunk, s);
  return fa2d::launch_decode<128>(q, k_cache, v_cache, seqlens, o, lse, workspace, B, H, Nmax, p.splits, p.chunk, s);
}

// describe hook (cln_describe, describe.hip; dims B, H, Nmax, D): CLN_ERR_BAD_ARG when `name` is not the entry
int cln_fa_decode_describe(const char* name, int B, int H, int Nmax, int D, int stages, char* buf, int len) {
  (void)stages;
  if (strcmp(name, "cln_fa2_decode") != 0) return CLN_ERR_BAD_ARG;
  DecodePlan p;
  const int rc = decode_plan(B, H, Nmax, D, &p);
  if (rc != CLN_OK) return rc;
  int n = snprintf(buf, len, "fa2_decode<D=%d> S=%d C=%d: 4 waves stream %d-key steps of K and V rows to registers, fp32 scores, online softmax", D,
                   p.splits, p.chunk, fa2d::key_step(D));
  if (p.splits > 1 && n < len)
    n += snprintf(buf + n, len - n, "; then fa2_decode_combine<D=%d> merges the live splits of a head by log-sum-exp in ascending order (workspace %lld bytes)",
                  D, p.ws_bytes);
  if (n < len) n += snprintf(buf + n, len - n, "; deterministic [one pipeline: stages ignored]");
  return n < len ? n : len - 1;
}
