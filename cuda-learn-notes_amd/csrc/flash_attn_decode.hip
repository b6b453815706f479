// Compile unit of the decode attention entries cln_fa2_decode_plan / cln_fa2_decode (include/cln_amd_ext.h; kernels: flash_attn_decode.cuh).
#include "flash_attn_decode.cuh"
#include <string.h>

namespace {

// The split plan (fa2d::split_plan): a function of (B, H, Nmax, D) only.
int decode_plan(int B, int H, int Nmax, int D, fa2d::Plan* p) {
  if (B <= 0 || H <= 0 || Nmax <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  return fa2d::split_plan((long long)B * H, (long long)B * H, Nmax, fa2d::key_step(D), D, p);
}

}  // namespace

CLN_API int cln_fa2_decode_plan(int B, int H, int Nmax, int D, int* splits, int* chunk, long long* workspace_bytes) {
  fa2d::Plan p;
  return fa2d::plan_out(decode_plan(B, H, Nmax, D, &p), p, splits, chunk, workspace_bytes);
}

CLN_API int cln_fa2_decode(const void* q, const void* k_cache, const void* v_cache, const int* seqlens, void* o, float* lse, void* workspace,
                           long long workspace_bytes, int B, int H, int Nmax, int D, void* stream) {
  const void* in[] = {q, k_cache, v_cache, seqlens};
  int rc = fa2d::check_pointers(in, 4, 3, {o, lse, workspace});
  if (rc != CLN_OK) return rc;
  fa2d::Plan p;
  rc = decode_plan(B, H, Nmax, D, &p);
  if (rc != CLN_OK) return rc;
  if (!fa2d::workspace_fits(p, workspace, workspace_bytes)) return CLN_ERR_BAD_ARG;
  const fa2d::DenseKV kv = {(const half_t*)k_cache, (const half_t*)v_cache, H, Nmax};
  const hipStream_t s = (hipStream_t)stream;
  if (D == 64) return fa2d::launch_decode<64, 1>(q, kv, seqlens, o, lse, workspace, B, p.splits, p.chunk, s);
  return fa2d::launch_decode<128, 1>(q, kv, seqlens, o, lse, workspace, B, p.splits, p.chunk, s);
}

// describe hook (cln_describe, describe.hip; dims B, H, Nmax, D): CLN_ERR_BAD_ARG when `name` is not the entry
int cln_fa_decode_describe(const char* name, int B, int H, int Nmax, int D, int stages, char* buf, int len) {
  (void)stages;
  if (strcmp(name, "cln_fa2_decode") != 0) return CLN_ERR_BAD_ARG;
  fa2d::Plan p;
  const int rc = decode_plan(B, H, Nmax, D, &p);
  if (rc != CLN_OK) return rc;
  const int n = snprintf(buf, len, "fa2_decode<D=%d> S=%d C=%d: 4 waves stream %d-key steps of K and V rows to registers, fp32 scores, online softmax",
                         D, p.splits, p.chunk, fa2d::key_step(D));
  return fa2d::describe_tail(buf, len, n, p, D, "head", " [one pipeline: stages ignored]");
}
