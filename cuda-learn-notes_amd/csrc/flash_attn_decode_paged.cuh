// Single-query ("decode") attention over a PAGED KV cache with grouped query heads:
//   O[b,h,:] = sum_{j < len_b} softmax_j(q[b,h] . K_j / sqrt(D)) V_j,  key j of sequence b and query head h = row j % page of KV head h / G in the
//   physical page block_table[b, j / page].
// q, o fp16 [B,Hq,D]; k_pages / v_pages fp16 [P,Hkv,page,D]; block_table int32 [B,max_pages] and seqlens int32 [B] ON THE DEVICE (the host reads
// neither). Hq = G Hkv, page a power of two (a run-time shift), the lengths clamped to [0, max_pages page] by the kernels.
//
// The kernel is fa2d::fa2_decode_kernel<D, G, PagedKV> (flash_attn_decode.cuh): the rows of one head in one page are consecutive in
// memory, so a wave load still covers 1 KiB of consecutive rows wherever the page is at least that long. A lane resolves each logical row to
// (physical page, offset) through the block table (fa2d::PagedKV). Only entries 0 .. ceil(len_b / page) - 1 of a sequence and only rows < len_b
// of the pages they name are addressed; the entries must lie in [0, P): that is the caller's contract, like the pointers.
#pragma once
#include "flash_attn_decode.cuh"

namespace fa2d {

// S splits of C keys (C a multiple of max(page, key_step(D)), S C >= max_pages page > (S - 1) C: the callers check it)
template <int D>
int launch_decode_paged(int G, const void* q, const PagedKV& kv, const int* seqlens, void* o, float* lse, void* workspace, int B, int S, int C,
                        hipStream_t stream) {
  switch (G) {
    case 1: return launch_decode<D, 1>(q, kv, seqlens, o, lse, workspace, B, S, C, stream);
    case 2: return launch_decode<D, 2>(q, kv, seqlens, o, lse, workspace, B, S, C, stream);
    case 4: return launch_decode<D, 4>(q, kv, seqlens, o, lse, workspace, B, S, C, stream);
    default: return launch_decode<D, 8>(q, kv, seqlens, o, lse, workspace, B, S, C, stream);
  }
}

}  // namespace fa2d
