// TEST-ONLY compile unit: the decode attention kernels (flash_attn_decode.cuh) with an EXPLICIT split plan, for the sweep that chose the
// constants of the product's plan (tools/fa_decode_probe.py, profiles/r11_fa_decode_probe.log). Linked into the probe library only.
#include "flash_attn_decode.cuh"

// As cln_fa2_decode, but S splits of C keys as given: C a multiple of the key step, S C >= Nmax > (S - 1) C, and for S > 1 a workspace of
// B H S (D + 2) 4 bytes. Returns the statuses of cln_fa2_decode; -2 for a plan that breaks these rules.
CLN_API int cln_fa2_decode_variant(const void* q, const void* k_cache, const void* v_cache, const int* seqlens, void* o, float* lse, void* workspace,
                                   long long workspace_bytes, int B, int H, int Nmax, int D, int S, int C, void* stream) {
  if (!q || !k_cache || !v_cache || !seqlens || !o || B <= 0 || H <= 0 || Nmax <= 0) return CLN_ERR_BAD_ARG;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  if (S <= 0 || C <= 0 || C % fa2d::key_step(D) != 0 || (long long)S * C < Nmax || (long long)(S - 1) * C >= Nmax) return CLN_ERR_UNSUPPORTED;
  if ((long long)B * H > 0x7fffffffLL || !fa2d::grid_fits((long long)B * H * S, (long long)B * H, D)) return CLN_ERR_UNSUPPORTED;
  if (S > 1 && (!workspace || workspace_bytes < fa2d::workspace_bytes((long long)B * H, S, D))) return CLN_ERR_BAD_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const fa2d::DenseKV kv = {(const half_t*)k_cache, (const half_t*)v_cache, H, Nmax};
  if (D == 64) return fa2d::launch_decode<64, 1>(q, kv, seqlens, o, lse, workspace, B, S, C, s);
  return fa2d::launch_decode<128, 1>(q, kv, seqlens, o, lse, workspace, B, S, C, s);
}
