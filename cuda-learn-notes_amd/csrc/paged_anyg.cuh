// What the four any-group-size paged attention kernels share and their power-of-two siblings do not have (the *_anyg_* headers):
// the map from row r of the T G query rows of a (sequence, KV head) to its token. Its head within the group is r - tok_of(r, G) G.
#pragma once

namespace fa2pp {

// the token r / G of row r >= 0: a plain unsigned 32-bit division, exact for every r < 2^32; used in front of and behind a key loop, never in it
__device__ __forceinline__ int tok_of(int r, int G) { return (int)((unsigned)r / (unsigned)G); }

}  // namespace fa2pp
