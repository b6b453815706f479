// Compile unit of the MoE expert sort: cln_moe_sort_plan, cln_moe_sort and their describe entries (include/cln_amd_ext.h; kernels:
// moe_sort.cuh). Status, in this order: a non-positive n_slots or E (-1); E > 65535 or a workspace of more than 2^28 ints
// (-2); a missing, misaligned (4 bytes) or aliased pointer, the workspace among them when the plan needs one (-1).
#include "moe_sort.cuh"

struct SortPlan {
  int blocks;
  long long ws_bytes;
};

static int sort_plan(int n_slots, int E, SortPlan* p) {
  if (n_slots < 1 || E < 1) return CLN_ERR_BAD_ARG;
  if (E > moe::kSortMaxE) return CLN_ERR_UNSUPPORTED;
  p->blocks = (int)(((long long)n_slots + moe::kChunk - 1) / moe::kChunk);
  p->ws_bytes = p->blocks == 1 ? 0 : 4LL * p->blocks * E;
  return p->ws_bytes <= (4LL << 28) ? CLN_OK : CLN_ERR_UNSUPPORTED;
}

static int sort_bits(int E) {
  int bits = 0;
  while ((1 << bits) < (E < moe::kTile ? E : moe::kTile)) ++bits;
  return bits;
}

CLN_API int cln_moe_sort_plan(int n_slots, int E, int* blocks, int* chunk, long long* workspace_bytes) {
  SortPlan p;
  const int rc = sort_plan(n_slots, E, &p);
  if (rc != CLN_OK) return rc;
  if (!blocks || !chunk || !workspace_bytes) return CLN_ERR_BAD_ARG;
  *blocks = p.blocks, *chunk = moe::kChunk, *workspace_bytes = p.ws_bytes;
  return CLN_OK;
}

CLN_API int cln_moe_sort(const int* topk_ids, int* expert_offsets, int* src, int* pos, void* workspace, int n_slots, int E, void* stream) {
  SortPlan p;
  const int rc = sort_plan(n_slots, E, &p);
  if (rc != CLN_OK) return rc;
  const void* ptr[5] = {topk_ids, expert_offsets, src, pos, workspace};
  const int np = p.blocks == 1 ? 4 : 5;
  for (int i = 0; i < np; ++i) {
    if (!ptr[i] || !cln_aligned(ptr[i], 4)) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < i; ++j)
      if (ptr[i] == ptr[j]) return CLN_ERR_BAD_ARG;
  }
  const moe::SortArgs a = {topk_ids, expert_offsets, src, pos, (int*)workspace, n_slots, E, sort_bits(E)};
  const dim3 grid((unsigned)p.blocks), block(moe::kSortThreads);
  if (p.blocks == 1) {
    CLN_LAUNCH(moe::moe_sort_rank<true>, grid, block, 0, (hipStream_t)stream, a);
    return cln_check_launch();
  }
  CLN_LAUNCH(moe::moe_sort_hist, grid, block, 0, (hipStream_t)stream, a);
  int st = cln_check_launch();
  if (st != CLN_OK) return st;
  CLN_LAUNCH(moe::moe_sort_scan, dim3(1), block, 0, (hipStream_t)stream, a, p.blocks);
  st = cln_check_launch();
  if (st != CLN_OK) return st;
  CLN_LAUNCH(moe::moe_sort_rank<false>, grid, block, 0, (hipStream_t)stream, a);
  return cln_check_launch();
}

static int sort_describe(const char* entry, int n_slots, int E, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  SortPlan p;
  const int rc = sort_plan(n_slots, E, &p);
  if (rc != CLN_OK) return rc;
  const int tiles = (E + moe::kTile - 1) / moe::kTile;
  int n;
  if (p.blocks == 1)
    n = snprintf(buf, len,
                 "%s n_slots=%d E=%d: blocks 1, chunk %d slots, 1 launch, no workspace: moe_sort_rank<one>, grid 1 workgroup of 256 threads, 32784 "
                 "bytes LDS static (4 wave histograms of %d experts), 0 bytes scratch, no spill, no global atomics; %d expert tile(s); a wave "
                 "owns 512 consecutive slots in 8 rounds of 64, peers by %d ballots an id, rank = the wave's running count + popcount of the "
                 "lower peers, a block scan over experts and waves in LDS gives expert_offsets and every row; stable; deterministic",
                 entry, n_slots, E, moe::kChunk, moe::kTile, tiles, sort_bits(E));
  else
    n = snprintf(buf, len,
                 "%s n_slots=%d E=%d: blocks %d, chunk %d slots, 3 launches on the stream, workspace %lld bytes (int32 [blocks][E]): moe_sort_hist "
                 "(grid %d workgroups of 256 threads, 8192 bytes LDS: a chunk's histogram by LDS adds), moe_sort_scan (grid 1 workgroup: per "
                 "expert the exclusive prefix over chunks in place, then over experts -> expert_offsets), moe_sort_rank<many> (grid %d "
                 "workgroups, 32768 bytes LDS static: each recomputes the ranks of its chunk and adds expert_offsets[e] + workspace[b][e]); 0 "
                 "bytes scratch, no spill, no global atomics, no workgroup waits on another inside a launch; %d expert tile(s), %d ballots an "
                 "id; stable; deterministic",
                 entry, n_slots, E, p.blocks, moe::kChunk, p.ws_bytes, p.blocks, p.blocks, tiles, sort_bits(E));
  return n < len ? n : len - 1;
}

CLN_API int cln_moe_sort_describe(int n_slots, int E, char* buf, int len) { return sort_describe("moe_sort", n_slots, E, buf, len); }
CLN_API int cln_moe_sort_plan_describe(int n_slots, int E, char* buf, int len) { return sort_describe("moe_sort_plan", n_slots, E, buf, len); }
