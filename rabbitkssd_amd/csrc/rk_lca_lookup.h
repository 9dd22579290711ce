// rk_lca_lookup.h -- the posting list of a query hash: the bucket of the prefix directory, then a binary search among the distinct hashes
// of the index, the kTrips searches of a lane advancing together (one probe of each per step: the loads of a step are in flight at once).
// The look-up of k_mask_flag (rk_mask.hip), which keeps its own copy: this header is used by rk_lca.hip and rk_screen.hip.
#pragma once
#include <cstdint>

struct LcaLookup {
    const void *uhash;        // Hash[U]: the index's distinct hashes, ascending
    const uint32_t *dir;      // u32[2^dir_bits + 1]
    unsigned long long U;     // 0: nothing is looked up
    int32_t hash_bits, dir_shift;
};

constexpr uint32_t kNoList = 0xFFFFFFFFu;

// list[t] = the index of the posting list of h[t], kNoList without one (in[t] false, a hash at or beyond 2^hash_bits, U == 0)
template <class Hash, int kTrips>
__device__ __forceinline__ void lca_lookup(const LcaLookup &ix, const unsigned long long (&h)[kTrips], const bool (&in)[kTrips], uint32_t (&list)[kTrips])
{
    const Hash *uhash = (const Hash *)ix.uhash;
    uint32_t lo[kTrips], hi[kTrips], end[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        // (a hash beyond the index's bits has no bucket; without distinct hashes there is no directory)
        const bool look = in[t] && ix.U && (ix.hash_bits >= 64 || (h[t] >> ix.hash_bits) == 0);
        lo[t] = hi[t] = 0;
        if (look) {
            const uint32_t b = (uint32_t)(h[t] >> ix.dir_shift);
            lo[t] = ix.dir[b];
            hi[t] = ix.dir[b + 1];
        }
        end[t] = hi[t];
    }
    for (bool more = true; more;) {
        more = false;
#pragma unroll
        for (int t = 0; t < kTrips; t++)
            if (lo[t] < hi[t]) {
                const uint32_t mid = (lo[t] + hi[t]) >> 1;   // (mid < hi <= dir[b + 1] <= U)
                if ((unsigned long long)uhash[mid] < h[t]) lo[t] = mid + 1; else hi[t] = mid;
                more |= lo[t] < hi[t];
            }
    }
#pragma unroll
    for (int t = 0; t < kTrips; t++)
        list[t] = lo[t] < end[t] && (unsigned long long)lo[t] < ix.U && (unsigned long long)uhash[lo[t]] == h[t] ? lo[t] : kNoList;
}
