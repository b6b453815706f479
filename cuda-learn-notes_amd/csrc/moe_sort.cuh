// The expert sort of a mixture-of-experts layer (cln_moe_sort, include/cln_amd_ext.h): topk_ids int32 [n_slots] (slot s =
// t k + j) -> expert_offsets int32 [E + 1] (exclusive prefix of the live counts), src int32 [n_slots] (sorted row -> slot, -1 from off[E]
// on) and pos int32 [n_slots] (slot -> sorted row, -1 for a dropped slot: an id outside [0, E)). A stable counting sort: within an expert
// the rows are in ascending slot. No global atomics, and no workgroup ever waits on another inside a launch.
//
// A workgroup of 256 threads owns a chunk of kChunk = 2048 consecutive slots: wave w the 512 slots from 512 w on, in 8 rounds of 64, lane =
// slot inside the round, so "earlier slot" is (wave, round, lane) order. The ids stay in 8 registers. Per tile of kTile = 2048 experts:
//   rank    per round the lanes with the same id find each other by ballots over the id's bits; a slot's rank inside its wave is the wave's
//           running count cnt[w][e] (LDS, touched by wave w alone) plus the popcount of its lower peers; the lowest peer adds the group's
//           size to cnt[w][e]. After 8 rounds cnt[w][.] is the wave's histogram.
//   scan    thread t owns experts 8 t ... 8 t + 7 of the tile: cnt[w][e] becomes base_e + the counts of the waves below w, with base_e the
//           exclusive prefix over experts (ONE workgroup: computed here with a block scan, and written to expert_offsets) or
//           expert_offsets[e] + the counts of the chunks below (workspace[b][e], written by the two launches before).
//   store   row = cnt[w][e] + rank; src[row] = slot, pos[slot] = row.
// blocks == 1 is that one launch. Otherwise three: moe_sort_hist (LDS histogram of a chunk -> workspace[b][E]), moe_sort_scan (one workgroup:
// per expert the exclusive prefix over chunks in place, then the prefix over experts -> expert_offsets), moe_sort_rank<false>.
#pragma once
#include "common.h"

namespace moe {

constexpr int kSortThreads = 256, kChunk = 2048, kTile = 2048, kSortRounds = kChunk / kSortThreads;
constexpr int kSortMaxE = 65535;

struct SortArgs {
  const int* ids;
  int *offsets, *src, *pos, *ws;
  int n, E, bits;  // bits: of min(E, kTile) - 1
};

// exclusive prefix of v over the 256 threads of the workgroup (thread order); *total = the sum. tmp holds 4 ints. Two barriers.
__device__ __forceinline__ int sort_block_scan(int v, int* tmp, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();  // tmp may still be read from the call before
  if (lane == 63) tmp[w] = inc;
  __syncthreads();
  int below = 0, all = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tmp[i];
    below += i < w ? c : 0;
    all += c;
  }
  *total = all;
  return below + inc - v;
}

__global__ __launch_bounds__(kSortThreads) void moe_sort_hist(const SortArgs a) {
  __shared__ int hist[kTile];
  const long long c0 = (long long)blockIdx.x * kChunk;
  int id[kSortRounds];
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const long long s = c0 + r * kSortThreads + threadIdx.x;
    id[r] = s < a.n ? a.ids[s] : -1;
  }
  for (int e0 = 0; e0 < a.E; e0 += kTile) {
    const int ne = min(kTile, a.E - e0);
    for (int e = threadIdx.x; e < ne; e += kSortThreads) hist[e] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
      if ((unsigned)(id[r] - e0) < (unsigned)ne) atomicAdd(&hist[id[r] - e0], 1);  // LDS; integer counts: any order gives the same sum
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ne; e += kSortThreads) a.ws[(size_t)blockIdx.x * a.E + e0 + e] = hist[e];
    __syncthreads();
  }
}

// one workgroup: ws[b][e] := sum of ws[b'][e] over b' < b; offsets[e] := exclusive prefix over experts of the column sums; offsets[E] := all
__global__ __launch_bounds__(kSortThreads) void moe_sort_scan(const SortArgs a, int blocks) {
  __shared__ int tmp[4];
  int running = 0;
  for (int e0 = 0; e0 < a.E; e0 += kSortThreads) {
    const int e = e0 + threadIdx.x;
    int acc = 0;
    if (e < a.E) {
      int b = 0;
      for (; b + 4 <= blocks; b += 4) {  // four loads in flight
        int* p = a.ws + (size_t)b * a.E + e;
        const int v0 = p[0], v1 = p[(size_t)a.E], v2 = p[2 * (size_t)a.E], v3 = p[3 * (size_t)a.E];
        p[0] = acc, p[(size_t)a.E] = acc + v0, p[2 * (size_t)a.E] = acc + v0 + v1, p[3 * (size_t)a.E] = acc + v0 + v1 + v2;
        acc += v0 + v1 + v2 + v3;
      }
      for (; b < blocks; ++b) {
        int* p = a.ws + (size_t)b * a.E + e;
        const int v = *p;
        *p = acc;
        acc += v;
      }
    }
    int total;
    const int ex = sort_block_scan(acc, tmp, &total);
    if (e < a.E) a.offsets[e] = running + ex;
    running += total;
  }
  if (threadIdx.x == 0) a.offsets[a.E] = running;
}

template <bool ONE>
__global__ __launch_bounds__(kSortThreads) void moe_sort_rank(const SortArgs a) {
  __shared__ int cnt[4][kTile];
  __shared__ int tmp[ONE ? 4 : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  const long long c0 = (long long)blockIdx.x * kChunk + w * (kChunk / 4) + lane;
  int id[kSortRounds], rank[kSortRounds];
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const long long s = c0 + 64 * r;
    id[r] = s < a.n ? a.ids[s] : -1;
    rank[r] = 0;
    if (s < a.n && (unsigned)id[r] >= (unsigned)a.E) a.pos[s] = -1;  // a dropped slot
  }
  int running = 0;  // ONE: the live slots of the tiles before
  for (int e0 = 0; e0 < a.E; e0 += kTile) {
    const int ne = min(kTile, a.E - e0);
    for (int e = threadIdx.x; e < ne; e += kSortThreads) cnt[0][e] = 0, cnt[1][e] = 0, cnt[2][e] = 0, cnt[3][e] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
      const int x = id[r] - e0;
      const bool in = (unsigned)x < (unsigned)ne;
      unsigned long long peers = __ballot(in);
      for (int b = 0; b < a.bits; ++b) {
        const bool bit = (x >> b) & 1;
        const unsigned long long m = __ballot(in && bit);
        peers &= bit ? m : ~m;
      }
      if (in) {
        const int old = cnt[w][x];
        rank[r] = old + __popcll(peers & lower);
        __builtin_amdgcn_wave_barrier();  // every peer has read before the lowest one writes: nothing may be scheduled across this point
        if ((peers & lower) == 0) cnt[w][x] = old + __popcll(peers);
      }
      __builtin_amdgcn_wave_barrier();  // the next round's reads, from other lanes, come after this round's writes (in-order LDS)
    }
    __syncthreads();
    int c[8][4], sum = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = 8 * threadIdx.x + i;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        c[i][v] = e < ne ? cnt[v][e] : 0;
        sum += c[i][v];
      }
    }
    int total = 0, base = 0;
    if (ONE) base = running + sort_block_scan(sum, tmp, &total);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = 8 * threadIdx.x + i;
      if (e < ne) {
        if (ONE) a.offsets[e0 + e] = base;
        else base = a.offsets[e0 + e] + a.ws[(size_t)blockIdx.x * a.E + e0 + e];
        cnt[0][e] = base;
        cnt[1][e] = base + c[i][0];
        cnt[2][e] = base + c[i][0] + c[i][1];
        cnt[3][e] = base + c[i][0] + c[i][1] + c[i][2];
        base += c[i][0] + c[i][1] + c[i][2] + c[i][3];
      }
    }
    running += total;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
      const int x = id[r] - e0;
      if ((unsigned)x < (unsigned)ne) {
        const int row = cnt[w][x] + rank[r];
        if ((unsigned)row < (unsigned)a.n) {  // always, when the ids did not change between the launches
          a.src[row] = (int)(c0 + 64 * r);
          a.pos[c0 + 64 * r] = row;
        }
      }
    }
    __syncthreads();
  }
  // the rows of no slot: each workgroup fills those of its own row range
  int live = running;
  if (ONE) {
    if (threadIdx.x == 0) a.offsets[a.E] = running;
  } else {
    live = a.offsets[a.E];
  }
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const long long row = (long long)blockIdx.x * kChunk + r * kSortThreads + threadIdx.x;
    if (row < a.n && row >= live) a.src[row] = -1;
  }
}

}  // namespace moe
